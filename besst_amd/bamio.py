"""BAM or SAM file -> resident records through the library's own readers (no pysam, no htslib).

This is the front-end the reference gets from ``pysam.Samfile(param.bamfile, 'rb')`` (runBESST:162): header
references/lengths plus, per record, exactly the attributes the hot path reads.  A BAM is inflated and decoded on the
device (or on host threads); the decoded columns are the same SoA layout the device kernels consume.

SAM text - what ``bwa mem``, ``bowtie2`` and ``minimap2`` print - is read by :class:`ResidentSam`: the header on the
host, the record lines parsed on the device (csrc/sam.hip) into the same columns, with the values the BAM of the same
records gives.  The file may be plain, BGZF or gzip; :func:`open_bam` tells the format by content, never by name.  Every
form is streamed in chunks - BGZF is inflated on the device and cut at line ends there (besst_dev_sam_lines), other gzip
is inflated by zlib on the host -, so the file may be of any size.  The record loop is exact on any record order, so an
aligner's read-ordered SAM goes straight in.
"""
import os
import zlib

import numpy as np

from . import _lib
from .records import RecordBatch


def reader_threads():
    """Workers of the reader's pool: twice the CPUs the process may use (_lib.effective_cpus: affinity and cgroup quota -
    a worker blocked in a page fault leaves its share unused), at most 128."""
    return min(128, 2 * _lib.effective_cpus())


def _open(lib, path, threads):
    handle = lib.besst_bam_open(os.fsencode(path), int(threads))
    if not handle:
        raise IOError('cannot read BAM %s: %s' % (path, _lib.last_error()))
    names, lengths = _header(lib, handle)
    return handle, names, lengths


def _header(lib, handle):
    """(reference names, lengths) of an open reader; the names in one call (a C5 header has 2 M of them)."""
    n_ref = lib.besst_bam_n_references(handle)
    need = lib.besst_bam_reference_names(handle, None, 0)
    buf = np.zeros(max(int(need), 1), dtype=np.uint8)
    lib.besst_bam_reference_names(handle, _lib.ptr(buf), int(need))
    names = buf[:need].tobytes().decode().split('\0')[:n_ref] if n_ref else []
    lengths = np.zeros(max(n_ref, 1), dtype=np.int32)
    _lib.check(lib.besst_bam_reference_lengths(handle, _lib.ptr(lengths)), 'bam_reference_lengths')
    return names, lengths[:n_ref].tolist()


class ResidentBam(object):
    """A BAM file whose records went straight to HBM - besst_ctx_push_bam_device: the compressed file is uploaded and
    inflated + decoded on the GPU (any BGZF block layout); else besst_ctx_push_bam: decode on host threads, pinned
    staging, copies under the next chunk's decode; ``mode`` as in GraphContext.push_bam - the `bam_file` argument for libmetrics.get_metrics and CreateGraph.PE when nothing
    on the host needs the record columns; ``part=(r, W)``: rank r's slice of the stream (htslib's layout; with ``first_skip`` - -1: guess, >= 0: inflated bytes in front of the slice's first record - the SLICE form for any block layout, ``boundary`` = (offset used, bytes of the last record in the next slice): distributed.ingest_slice runs the check between ranks; multi-GPU ingest: ``len()`` and the
    head arrays then describe that slice only - such an object is for distributed.ingest_slice, not for
    libmetrics.get_metrics, whose < 1000-record check and read-length step are about the whole file).  It carries what the host side of those two does read: the header
    (``references``, ``lengths``), the record count (``len()``) and ``rlen`` / ``alen`` / ``qlen`` of the first 1000
    records (the read-length step, libmetrics.py:246-273); ``ctx`` is the GraphContext that holds the records and
    ``ingest`` the timings of the upload."""

    def __init__(self, path, device_index=0, threads=None, chunk_records=4 << 20, mode=None, chunk_blocks=0, part=None,
                 first_skip=None):
        from . import device
        lib = _lib.load()
        threads = threads or reader_threads()
        handle, self.references, self.lengths = _open(lib, path, threads)
        self.path = path
        self.ctx = None
        try:
            self.ctx = device.GraphContext(device_index)     # (inside the try: a context that cannot be made must not leak the reader)
            zeros = np.zeros(len(self.references), dtype=np.int32)
            self.ctx.set_contigs(scaf_id=zeros, scaf_len=zeros, ctg_pos=zeros, ctg_len=zeros, direction=zeros, cls=zeros)
            self.ingest, self.rlen, self.alen, self.qlen = self.ctx.push_bam(handle, chunk_records, mode=mode, chunk_blocks=chunk_blocks, part=part,
                                                                              first_skip=first_skip)
            self.boundary = getattr(self.ctx, 'slice_boundary', None)
            clamped = lib.besst_bam_clamped_records(handle)
        except Exception:
            if self.ctx is not None:
                self.ctx.close()
            raise
        finally:
            lib.besst_bam_close(handle)
        self._n = int(self.ingest.records)
        if clamped > 0:
            import warnings
            warnings.warn('%s: %d record(s) align more than 65535 query bases; their qlen is stored as 65535' % (path, clamped))

    def __len__(self):
        return self._n

    def layout_state(self):
        """GraphContext.layout_state(): after a device ingest the bit planes and the candidate side stream of the records are
        there already (all three watermarks at ``len()``), and the first build launches no maker."""
        return self.ctx.layout_state()

    def report(self, isize_bins=32768):
        """The BAM report of the file (GraphContext.library_report, besst_amd.report) with the header's names and lengths.
        Over a ``part`` it describes that slice."""
        rep = self.ctx.library_report(isize_bins)
        rep.references, rep.lengths = list(self.references), [int(x) for x in self.lengths]
        return rep

    def close(self):
        self.ctx.close()


class ShardedBam(object):
    """The `bam_file` argument of libmetrics.get_metrics / CreateGraph.PE under a process group (one process per GPU):
    this rank's slice of the file, inflated and decoded on its GPU (distributed.ingest_slice: any BGZF block layout, the
    ranks settle where each slice's first record begins), plus what the host side reads of the whole file - header,
    global record count, rlen / alen / qlen of the stream's first 1000 records (sharded.ShardedHead).  ``ingest``: the
    slice's timings."""

    def __init__(self, path, group=None, device_index=None, threads=None, chunk_blocks=0):
        import torch
        import torch.distributed as dist
        from . import distributed, pipeline, sharded
        self.path, self.group = path, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        dev = torch.cuda.current_device() if device_index is None else int(device_index)
        self.slice, cols = distributed.ingest_slice(path, self.rank, self.world, device_index=dev, threads=threads,
                                                    chunk_blocks=chunk_blocks, group=group)
        self.ingest = self.slice.ingest
        self.references, self.lengths = self.slice.references, self.slice.lengths
        device = torch.device('cuda', dev)
        rec = pipeline.DeviceRecords.from_columns(cols)
        self.engine = sharded.HipRankEngine(device, rec, len(self.references), keep=self.slice)
        self.head = sharded.ShardedHead(self.references, self.lengths, len(self.slice),
                                        (self.slice.rlen, self.slice.alen, self.slice.qlen), group, self.world)
        self.rlen, self.alen, self.qlen = self.head.rlen, self.head.alen, self.head.qlen

    def __len__(self):
        return len(self.head)

    def report(self, isize_bins=32768):
        """The BAM report of the WHOLE file on every rank (collective): each rank runs besst_dev_library_report over its
        slice, the words are summed over the group - the digest's xor word is gathered and xor-ed instead."""
        import torch
        import torch.distributed as dist
        from . import distributed, report, sharded
        words, err = None, None
        try:
            words = report.dev_report_tensor(self.engine.rec, len(self.references), isize_bins)
            xor_word = int(words[report.DIGEST_XOR].item())
            words[report.DIGEST_XOR] = 0
        except Exception as e:
            err = '%s: %s' % (type(e).__name__, e)
        sharded._agree(self.group, self.world, err)          # (nobody enters the all-reduce without the others)
        distributed._all_reduce(words, self.group)
        xors = [None] * self.world
        dist.all_gather_object(xors, xor_word, group=self.group)
        host = words.cpu().numpy().view(np.uint64).copy()
        for x in xors:
            host[report.DIGEST_XOR] ^= np.uint64(x & 0xffffffffffffffff)
        return report.LibraryReport(host, len(self.references), isize_bins, self.references, self.lengths)

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None


class SamError(ValueError):
    """A SAM file cannot be read.  ``offset``: the first byte of the line at fault (of the inflated text where the file is
    compressed), ``line``: its 1-based number or None, ``reason``: one of SAM_REASONS' words.  ``reason`` 'compressed
    data': the file's gzip / BGZF data is damaged; ``offset`` is then the block's or member's in the COMPRESSED file."""

    def __init__(self, message, offset, line=None, reason=None):
        ValueError.__init__(self, message)
        self.offset, self.line, self.reason = offset, line, reason


# include/besst_amd.h: BESST_SAM_*
SAM_REASONS = {1: 'fewer than eleven fields', 2: 'empty line', 3: 'header line behind a record', 4: 'FLAG is not a number in 0..65535',
               5: 'POS is not a number in 0..2^31-1', 6: 'MAPQ is not a number in 0..255', 7: 'PNEXT is not a number in 0..2^31-1',
               8: 'TLEN is not a number within int32', 9: 'RNAME is not among the references',
               10: 'RNEXT is not among the references', 11: 'CIGAR is malformed'}
GZIP_MAGIC = b'\x1f\x8b'
SAM_CHUNK_BYTES = 64 << 20               # ResidentSam streams a plain file through two pinned buffers of this size
SAM_DEFAULT_TILE = 16384                 # csrc/sam.hip: the tile of tile_bytes = 0
SAM_TEXT_PAD = 64                        # readable bytes behind a chunk's end in HBM
SAM_MAX_TEXT = (1 << 32) - 17            # one parsed chunk (besst_ctx_push_sam_text)
BGZF_MAX_ISIZE = 65536                   # a BGZF block inflates to this much at most
HEAD_RECORDS = 1000


def parse_sam_header(lines):
    """The header's lines (bytes, terminators included or not) -> (names, lengths): one reference per @SQ line in file
    order, SN: and LN: found among its tab-separated tags in any order; other lines are skipped.  SamError (offset of the
    line within the header, 1-based line): an @SQ without SN or LN, an LN that is no number in 0..2^31-1 (a BAM header may say 0, so 0 is taken), a repeated SN."""
    names, lengths, seen, at = [], [], set(), 0
    for no, raw in enumerate(lines, 1):
        line = raw.rstrip(b'\n')
        if line.endswith(b'\r'):
            line = line[:-1]
        fields = line.split(b'\t')
        if fields[0] == b'@SQ':
            sn = [f[3:] for f in fields[1:] if f.startswith(b'SN:')]
            ln = [f[3:] for f in fields[1:] if f.startswith(b'LN:')]
            if not sn or not ln or not sn[0]:
                raise SamError('@SQ line %d has no SN or no LN' % no, at, no, 'header')
            if not ln[0].isdigit() or int(ln[0]) >= (1 << 31):
                raise SamError('@SQ line %d: LN is not a length' % no, at, no, 'header')
            name = sn[0].decode('utf-8', 'surrogateescape')
            if name in seen:
                raise SamError('@SQ line %d repeats SN:%s' % (no, name), at, no, 'header')
            seen.add(name)
            names.append(name)
            lengths.append(int(ln[0]))
        at += len(raw)
    return names, lengths


def _read_plain_header(fh):
    """The leading run of '@' lines of an open binary file -> (lines, their bytes); the file stands behind them."""
    lines, size = [], 0
    while True:
        here = fh.tell()
        if fh.read(1) != b'@':
            fh.seek(here)
            return lines, size
        line = b'@' + fh.readline()
        lines.append(line)
        size += len(line)


def _sam_error(path, info, line, compressed):
    off, code = int(info[2]), int(info[3])
    reason = SAM_REASONS.get(code, 'reason %d' % code)
    where = ' of the inflated text (the file is compressed)' if compressed else ''
    return SamError('%s: %s at byte %d%s%s' % (path, reason, off, where, '' if line is None else ', line %d' % line),
                    off, line, reason)


class ResidentSam(object):
    """A SAM text file whose records went to HBM, parsed on the device (csrc/sam.hip): the interface of ResidentBam -
    ``references``, ``lengths``, ``ctx``, ``ingest``, ``rlen`` / ``alen`` / ``qlen`` of the first 1000 records, ``len()``,
    ``layout_state()``, ``report()``, ``close()`` - so that libmetrics.get_metrics and CreateGraph.PE take it unchanged.

    A plain file: the header is read on the host, the record lines stream through two pinned buffers of ``chunk_bytes``
    (a multiple of ``tile_bytes``), each chunk cut at its last line end and the tail carried to the front of the next one -
    only the columns stay resident, the file may be larger than HBM.  A file that begins with the gzip magic is streamed as
    well, ``chunk_bytes`` of inflated text a round: BGZF is inflated on the device into two text buffers, cut at
    its last line end by the device (``inflate`` 'device'; ``inflate_stats``: rounds, windows, host_rounds, host_from);
    other gzip is inflated by zlib on the host and goes through the plain file's loop ('host').  With ``gzip_on_gpu`` a gzip
    file whose text is below 4 GiB and fits in HBM is inflated there whole and parsed as one chunk ('device_gzip'); else it
    is streamed on the host and ``inflate_stats['status']`` says why ('too_large', 'allocation', or the device's reason).

    The mate / run planes and the candidate side stream are not written while decoding: ``layout_state()`` shows the
    watermarks at 0 and the first build runs the makers, as after a host push.  SamError: a line that cannot be read (the
    smallest offset wins); the context is then gone with its records."""

    def __init__(self, path, device_index=0, chunk_bytes=None, tile_bytes=None, gzip_on_gpu=False):
        import time
        from . import device
        tile = int(tile_bytes or 0)
        if tile and (tile % 1024 or not 1024 <= tile <= 65536):
            raise ValueError('tile_bytes must be a multiple of 1024 in 1024..65536')
        chunk = int(SAM_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        if chunk < (tile or SAM_DEFAULT_TILE) or chunk % (tile or SAM_DEFAULT_TILE) or chunk > SAM_MAX_TEXT:
            raise ValueError('chunk_bytes must be a multiple of tile_bytes, at least one tile and below 4 GiB')
        self.path, self.ctx = path, None
        self._lib = _lib.load()
        self._tile, self._saturated = tile, 0
        self.inflate, self.inflate_stats = None, None            # a compressed file: 'device', 'device_gzip' or 'host'
        self.ingest = _lib.IngestStats()
        self.ingest.on_device = 1
        self._head = (np.zeros(HEAD_RECORDS, dtype=np.int32), np.zeros(HEAD_RECORDS, dtype=np.int32),
                      np.zeros(HEAD_RECORDS, dtype=np.uint16))
        t0 = time.perf_counter()
        with open(path, 'rb') as fh:
            compressed = fh.read(2) == GZIP_MAGIC
        try:
            if compressed:
                self._read_compressed(device, int(device_index), bool(gzip_on_gpu), chunk)
            else:
                self._read_plain(device, int(device_index), chunk)
        except Exception:
            if self.ctx is not None:
                self.ctx.close()                                 # (clear_records and all: nothing half-pushed is used)
                self.ctx = None
            raise
        self.ingest.seconds = time.perf_counter() - t0
        self._n = int(self.ingest.records)
        k = min(HEAD_RECORDS, self._n)
        self.rlen, self.alen, self.qlen = (a[:k] for a in self._head)
        if self._saturated > 0:
            import warnings
            warnings.warn('%s: %d record(s) align more than 65535 query bases; their qlen is stored as 65535'
                          % (path, self._saturated))

    # ---- the header becomes the context --------------------------------------------------------------------------------
    def _open_context(self, device, device_index, header_lines):
        self.references, self.lengths = parse_sam_header(header_lines)
        self.ctx = device.GraphContext(device_index)
        zeros = np.zeros(len(self.references), dtype=np.int32)
        self.ctx.set_contigs(scaf_id=zeros, scaf_len=zeros, ctg_pos=zeros, ctg_len=zeros, direction=zeros, cls=zeros)
        blobs = [n.encode('utf-8', 'surrogateescape') for n in self.references]
        off = np.zeros(len(blobs) + 1, dtype=np.int64)
        np.cumsum(np.fromiter((len(b) for b in blobs), dtype=np.int64, count=len(blobs)), out=off[1:])
        pool = np.frombuffer(b''.join(blobs) or b'\0', dtype=np.uint8)
        _lib.check(self._lib.besst_ctx_set_sam_references(self.ctx._ctx, _lib.ptr(pool), _lib.ptr(off), len(blobs)),
                   'set_sam_references')

    def _push(self, stream, text_ptr, n_bytes, file_offset):
        """One chunk in HBM -> the context; -> info (records, saturated, error offset, reason)."""
        import ctypes as C
        info = np.zeros(4, dtype=np.int64)
        rlen, alen, qlen = self._head
        _lib.check(self._lib.besst_ctx_push_sam_text(self.ctx._ctx, C.c_void_p(stream), C.c_void_p(text_ptr), int(n_bytes),
                                                     int(file_offset), self._tile, HEAD_RECORDS, _lib.ptr(rlen), _lib.ptr(alen),
                                                     _lib.ptr(qlen), _lib.ptr(info)), 'push_sam_text')
        if info[2] < 0:
            self.ingest.records += int(info[0])
            self.ingest.chunks += 1
            self._saturated += int(info[1])
        return info

    # ---- a plain file: chunks through two pinned buffers -----------------------------------------------------------------
    def _read_plain(self, device, device_index, chunk):
        with open(self.path, 'rb') as fh:
            header, at = _read_plain_header(fh)
            self._open_context(device, device_index, header)
            left = os.fstat(fh.fileno()).st_size - at
            at = self._stream_lines(device_index, fh, len(header), at, left, chunk, False)
        self.ingest.inflated_bytes = at

    def _stream_lines(self, device_index, fh, lines_before, at, left, chunk, compressed):
        """The record lines that ``fh.readinto`` brings (a plain file behind its header, or the inflated bytes of gzip
        members), in chunks through two pinned buffers, into the open context.  ``at``: the text offset of the first of
        them, ``lines_before``: the lines in front; ``left``: their bytes where known (None: not known - the chunk is not
        made smaller and the columns are not announced).  -> the text offset behind the last byte."""
        import torch
        dev = torch.device('cuda', device_index)
        step = self._tile or SAM_DEFAULT_TILE
        if left is not None:                                 # (a file smaller than a chunk needs no more than its size)
            chunk = min(chunk, max(step, -(-left // step) * step))
            _lib.check(self._lib.besst_ctx_sam_expect_text(self.ctx._ctx, int(left)), 'sam_expect_text')
        with torch.cuda.device(dev):
            h_buf = [torch.empty(chunk, dtype=torch.uint8).pin_memory() for _ in range(2)]
            # (not zeroed: the parser masks every byte behind a chunk's end, the pad only has to be readable - and a
            # fill on the current stream would have to be ordered in front of the first copies on the side stream)
            d_buf = [torch.empty(chunk + SAM_TEXT_PAD, dtype=torch.uint8, device=dev) for _ in range(2)]
            views = [memoryview(b.numpy()) for b in h_buf]
            copy = torch.cuda.Stream(dev)
            copy.wait_stream(torch.cuda.current_stream(dev))
            pending = None                                # (slot, bytes, file offset, copied event) of the chunk in flight
            carry, slot, eof = 0, 0, False

            def parse(job):
                nonlocal lines_before
                j_slot, j_bytes, j_off, j_done = job
                torch.cuda.current_stream(dev).wait_event(j_done)
                info = self._push(torch.cuda.current_stream(dev).cuda_stream, d_buf[j_slot].data_ptr(), j_bytes, j_off)
                if info[2] >= 0:
                    rel = int(info[2]) - j_off
                    line = lines_before + 1 + int(np.count_nonzero(h_buf[j_slot].numpy()[:rel] == 10))
                    raise _sam_error(self.path, info, line, compressed)
                lines_before += int(info[0])

            try:
                while not eof:
                    view = views[slot]
                    room = chunk - carry
                    got = _read_full(fh, view[carry:chunk]) if room else 0
                    have = carry + got
                    eof = got < room
                    if have == 0:
                        break
                    cut = have if eof else _last_line_end(view, have)
                    if cut == 0:
                        if pending is not None:
                            parse(pending)                   # (an earlier line's error comes first)
                        raise SamError('%s: the line at byte %d is longer than chunk_bytes = %d; raise chunk_bytes'
                                       % (self.path, at, chunk), at, None, 'line longer than a chunk')
                    with torch.cuda.stream(copy):
                        d_buf[slot][:cut].copy_(h_buf[slot][:cut], non_blocking=True)
                        done = torch.cuda.Event()
                        done.record(copy)
                    self.ingest.bytes_h2d += cut
                    job = (slot, cut, at, done)
                    if pending is not None:
                        parse(pending)                       # chunk c - 1 is parsed while chunk c crosses
                    pending = job
                    other = views[1 - slot]                  # (its chunk was parsed just now: the buffer is free)
                    carry = have - cut
                    other[:carry] = view[cut:have]
                    at += cut
                    slot = 1 - slot
                if pending is not None:
                    parse(pending)
            finally:
                copy.synchronize()                           # no copy is in flight when the buffers are let go, error or not
        return at

    # ---- a compressed file: inflated and parsed chunk by chunk --------------------------------------------------------------
    def _compressed_error(self, message, offset):
        """(the offset is the damaged block's or member's in the COMPRESSED file - the text was never inflated that far)"""
        return SamError('%s: %s (byte %d of the compressed file, not of the inflated text)'
                        % (self.path, message.replace('compressed FASTA file', 'compressed SAM file'), offset),
                        offset, None, 'compressed data')

    def _read_compressed(self, device, device_index, gzip_on_gpu, chunk):
        from . import GenerateOutput as GO
        torch, dev = GO._torch_device(device_index)
        n_blocks, total, end, size = GO.bgzf_walk(self.path)
        try:
            if end > 0:                                          # the file begins with a chain of BGZF blocks
                with torch.cuda.device(dev):
                    self._read_bgzf(device, device_index, torch, dev, chunk, total, end, size)
                return
            stats = dict(chunks=0, candidates=0, live=0, text_bytes=0, status=None)
            self.inflate_stats = stats
            if gzip_on_gpu:
                with torch.cuda.device(dev):
                    got = GO._upload_gzip_device(torch, dev, self.path, GO.GZIP_CHUNK_BYTES, stats, max_text=SAM_MAX_TEXT)
                if got is not None:
                    self.inflate = 'device_gzip'
                    self.ingest.bytes_h2d = size
                    self.ingest.inflated_bytes = got[1]
                    self._parse_resident(device, device_index, torch, dev, got[0], got[1])
                    return
            self.inflate = 'host'
            with open(self.path, 'rb') as fh:
                self._read_members(device, device_index, fh, 0, b'', [], True, 0, chunk)
        except GO.FastaError as exc:                             # (the uploaders word their errors for the contig file)
            raise self._compressed_error(str(exc), exc.offset)

    def _read_members(self, device, device_index, fh, base, prefix, header, in_header, at, chunk):
        """The gzip members from byte ``base`` of the file on, inflated by zlib on the host and streamed as a plain file is.
        ``prefix``: text in front of their output (what a chain of BGZF blocks left behind its last cut), ``header``: the
        header lines read so far, ``in_header``: the header may go on, ``at``: the text offset of the prefix's first byte."""
        src = _MemberStream(fh, base, prefix)
        if in_header:
            more, size = src.header_lines()
            header, at = header + more, at + size
        if self.ctx is None:
            self._open_context(device, device_index, header)
        at = self._stream_lines(device_index, src, len(header) + int(self.ingest.records), at, None, chunk, True)
        self.ingest.inflated_bytes = at

    def _read_bgzf(self, device, device_index, torch, dev, chunk, total, end, size):
        """BGZF text, round by round.  A round: the text buffer holds the carry - the bytes behind the last
        cut - at offset 0; whole blocks are appended in file order while fewer than ``chunk`` bytes are held; they are
        inflated at their places (besst_dev_bgzf_inflate), the cutter (besst_dev_sam_lines) finds the last line end or the
        header's end, and one read brings its answers and the first bad block to the host.  The text up to the cut is
        pushed, the rest is copied to the front of the other buffer.  The compressed bytes come through two pinned and two
        device windows; the next window is read and sent while the round's kernels run."""
        import ctypes as C
        from . import GenerateOutput as GO
        lib, p = self._lib, C.c_void_p
        step = self._tile or SAM_DEFAULT_TILE
        chunk = min(chunk, (SAM_MAX_TEXT - BGZF_MAX_ISIZE) // step * step)
        if end == size:                                          # (a file smaller than a chunk needs no more than its text)
            chunk = min(chunk, max(step, -(-total // step) * step))
        self.inflate = 'device'
        stats = self.inflate_stats = dict(rounds=0, windows=0, host_rounds=0, host_from=None, status=None)
        main = torch.cuda.current_stream(dev)
        per_launch = int(GO.BLOCKS_PER_LAUNCH)
        launch_cap = min(per_launch * BGZF_MAX_ISIZE, chunk + BGZF_MAX_ISIZE)
        ws_bytes = lib.besst_dev_bgzf_inflate_workspace_bytes(per_launch, launch_cap)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        # (not zeroed: the cutter and the parser mask every byte behind the text's end, the pad only has to be readable)
        t_buf = [torch.empty(chunk + BGZF_MAX_ISIZE + SAM_TEXT_PAD, dtype=torch.uint8, device=dev) for _ in range(2)]
        status = torch.full((5,), -1, dtype=torch.int64, device=dev)      # the cutter's four words, the first bad block
        cap = min(max(GO.BGZF_MAX_BLOCK, min(int(GO.UPLOAD_CHUNK), chunk)), max(GO.BGZF_MAX_BLOCK, -(-end // 16) * 16))
        w_host = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        w_dev = [torch.zeros(cap + GO.BGZF_COMP_PAD, dtype=torch.uint8, device=dev) for _ in range(2)]
        w_view = [memoryview(b.numpy()) for b in w_host]
        desc_type = np.dtype([('src_off', '<u4'), ('src_len', '<u4'), ('dst_lo', '<u4'), ('dst_hi', '<u4'), ('dst_len', '<u4'),
                              ('crc', '<u4')])
        assert desc_type.itemsize == GO.BGZF_DESC_BYTES
        scan_cap = cap // 26 + 2                                 # (a block is 28 bytes at least)
        scanned = np.zeros(scan_cap, dtype=desc_type)
        d_cap = max(2 * per_launch, 8192)                        # descriptors staged per round (more: a wait in the middle)
        h_desc = torch.empty(d_cap * GO.BGZF_DESC_BYTES, dtype=torch.uint8).pin_memory()
        d_desc = torch.empty(d_cap * GO.BGZF_DESC_BYTES, dtype=torch.uint8, device=dev)
        h_desc_np = h_desc.numpy().view(desc_type)
        copy = torch.cuda.Stream(dev)
        copy.wait_stream(main)
        sent, inflated_ev = [None, None], [None, None]
        state = dict(file_at=0, cut_block=b'', w_slot=0, blocks=0)
        n_got, comp, infl = C.c_int64(0), C.c_size_t(0), C.c_int64(0)

        def more_windows():
            return state['file_at'] < end or len(state['cut_block']) > 0

        def load_window(fh):
            """the next window of the chain: read, its blocks found, sent on the side stream -> its table"""
            slot = state['w_slot']
            if sent[slot] is not None:
                sent[slot].synchronize()                         # the buffer's last copy has left it
            view, have = w_view[slot], len(state['cut_block'])
            first_at = state['file_at'] - have
            view[:have] = state['cut_block']
            want = min(cap - have, end - state['file_at'])
            got = _read_full(fh, view[have:have + want])
            if got != want:
                raise IOError('%s ended %d bytes early' % (self.path, want - got))
            have, state['file_at'] = have + got, state['file_at'] + got
            _lib.check(lib.besst_bgzf_scan_chunk(p(w_host[slot].data_ptr()), have, 0, 1 if state['file_at'] < end else 0, scan_cap, 0,
                                                 p(scanned.ctypes.data), C.byref(n_got), C.byref(comp), C.byref(infl)),
                       'besst_bgzf_scan_chunk')
            n = int(n_got.value)
            if not n:
                raise IOError('%s changed while it was read' % self.path)
            d = scanned[:n]
            src_off, src_len = d['src_off'].astype(np.int64), d['src_len'].astype(np.int64)
            starts = np.empty(n, dtype=np.int64)                 # where every block begins in the file
            starts[0] = first_at
            starts[1:] = first_at + src_off[:-1] + src_len[:-1] + 8
            tab = dict(slot=slot, n=n, at=0, src_off=d['src_off'].copy(), src_len=d['src_len'].copy(), isize=d['dst_len'].copy(),
                       crc=d['crc'].copy(), cum=np.cumsum(d['dst_len'].astype(np.int64)), starts=starts,
                       payload_at=first_at + src_off)
            state['cut_block'] = bytes(view[comp.value:have])
            with torch.cuda.stream(copy):
                if inflated_ev[slot] is not None:
                    copy.wait_event(inflated_ev[slot])           # the launches that last read this device window
                w_dev[slot][:comp.value].copy_(w_host[slot][:comp.value], non_blocking=True)
                sent[slot] = torch.cuda.Event()
                sent[slot].record(copy)
            self.ingest.bytes_h2d += int(comp.value)
            state['w_slot'] = 1 - slot
            stats['windows'] += 1
            return tab

        header, in_header, lines_before = [], True, 0
        text_at, carry, slot = 0, 0, 0
        cur, nxt = None, None
        tail = end < size                                        # something that is no BGZF block follows the chain
        try:
            with open(self.path, 'rb', buffering=0) as fh:
                while True:
                    # -- the round's blocks: launched as they are taken
                    held, first_block, used, taken = carry, state['blocks'], 0, []
                    while held < chunk:
                        if cur is None or cur['at'] == cur['n']:
                            if nxt is not None:
                                cur, nxt = nxt, None
                            elif more_windows():
                                cur = load_window(fh)
                            else:
                                cur = None
                                break
                            continue
                        cum, a = cur['cum'], cur['at']
                        before = int(cum[a - 1]) if a else 0
                        j = min(cur['n'], int(np.searchsorted(cum, before + chunk - held, side='left')) + 1)
                        main.wait_event(sent[cur['slot']])
                        while a < j:
                            before = int(cum[a - 1]) if a else 0
                            b = min(j, a + per_launch, int(np.searchsorted(cum, before + launch_cap, side='right')))
                            b = max(b, a + 1)
                            nb, nbytes = b - a, int(cum[b - 1]) - before
                            if used + nb > d_cap:
                                main.synchronize()               # the staged descriptors have been read
                                used = 0
                            d = h_desc_np[used:used + nb]
                            d['src_off'], d['src_len'] = cur['src_off'][a:b], cur['src_len'][a:b]
                            d['dst_len'], d['crc'], d['dst_hi'] = cur['isize'][a:b], cur['crc'][a:b], 0
                            d['dst_lo'] = (cum[a:b] - cur['isize'][a:b].astype(np.int64) - before).astype(np.uint32)
                            lo, hi = used * GO.BGZF_DESC_BYTES, (used + nb) * GO.BGZF_DESC_BYTES
                            d_desc[lo:hi].copy_(h_desc[lo:hi], non_blocking=True)
                            _lib.check(lib.besst_dev_bgzf_inflate(p(main.cuda_stream), p(w_dev[cur['slot']].data_ptr()),
                                                                  p(d_desc.data_ptr() + lo), nb, state['blocks'], nbytes,
                                                                  p(t_buf[slot].data_ptr() + held), p(ws.data_ptr()), ws_bytes,
                                                                  p(status.data_ptr() + 32)), 'besst_dev_bgzf_inflate')
                            taken.append((cur, a, b, held))
                            used, held, a = used + nb, held + nbytes, b
                            state['blocks'] += nb
                        cur['at'] = j
                        inflated_ev[cur['slot']] = torch.cuda.Event()
                        inflated_ev[cur['slot']].record(main)
                    chain_end = (cur is None or cur['at'] == cur['n']) and nxt is None and not more_windows()
                    eof = chain_end and not tail
                    if held == 0:
                        break
                    stats['rounds'] += 1
                    # -- the next window is read and sent while the round's kernels run
                    if nxt is None and more_windows() and (cur is None or cur['slot'] != state['w_slot']):
                        nxt = load_window(fh)
                    words = self._cut(main, t_buf[slot], held, in_header, 0, status)
                    if words[4] != -1:
                        block, reason = int(words[4]) >> 8, int(words[4]) & 0xff
                        k = block - first_block
                        for tab, a, b, _ in taken:
                            if k < b - a:
                                bad_at = int(tab['starts'][a + k])
                                break
                            k -= b - a
                        if reason in (GO.BGZF_BAD_SIZE, GO.BGZF_BAD_CRC):
                            raise self._compressed_error(
                                'the BGZF block at byte %d of the compressed SAM file (block %d) is damaged: %s' % (
                                    bad_at, block, 'its CRC-32 is not that of its inflated bytes' if reason == GO.BGZF_BAD_CRC
                                    else 'it does not inflate to ISIZE bytes'), bad_at)
                        # the device kernel does not take a block's DEFLATE data: the round's blocks by zlib on the host
                        self._host_round(torch, dev, taken, t_buf[slot])
                        stats['host_rounds'] += 1
                        status[4:].fill_(-1)
                        words = self._cut(main, t_buf[slot], held, in_header, 0, status)
                    last_end, header_end = int(words[0]), int(words[1])
                    if in_header and header_end != 0:
                        if header_end < 0:                       # header lines, the last one perhaps not whole
                            take = held if eof else last_end
                        else:
                            take, in_header = header_end, header_end == held
                        if take == 0 and held >= chunk:
                            raise self._long_line(text_at, chunk)
                        header += _split_lines(t_buf[slot][:take].cpu().numpy().tobytes())
                    else:
                        if in_header:
                            in_header = False
                        if self.ctx is None:
                            self._open_context(device, device_index, header)
                            lines_before = len(header)
                            if not tail:                         # an estimate: the whole text, the header's bytes included
                                _lib.check(lib.besst_ctx_sam_expect_text(self.ctx._ctx, int(total - text_at)), 'sam_expect_text')
                        take = held if eof else last_end
                        if take == 0 and held >= chunk:
                            raise self._long_line(text_at, chunk)
                        if take:
                            info = self._push(main.cuda_stream, t_buf[slot].data_ptr(), take, text_at)
                            if info[2] >= 0:
                                rel = int(info[2]) - text_at
                                words = self._cut(main, t_buf[slot], held, False, rel, status)
                                raise _sam_error(self.path, info, lines_before + int(self.ingest.records) + int(words[2]) + 1, True)
                    carry = held - take
                    if carry:
                        t_buf[1 - slot][:carry].copy_(t_buf[slot][take:held])
                    text_at, slot = text_at + take, 1 - slot
                    if chain_end and tail:
                        break
                self.ingest.inflated_bytes = text_at
                if tail:                                         # the rest of the file through zlib on the host
                    stats['host_from'] = int(end)
                    prefix = t_buf[slot][:carry].cpu().numpy().tobytes()
                    del t_buf, ws, w_dev
                    fh.seek(end)
                    self._read_members(device, device_index, fh, end, prefix, header, in_header, text_at, chunk)
                elif self.ctx is None:
                    self._open_context(device, device_index, header)     # a file of header lines alone
        finally:
            copy.synchronize()
            main.synchronize()                                   # nothing is in flight when the buffers are let go, error or not

    def _cut(self, main, text, n_bytes, want_header_end, count_upto, status):
        """besst_dev_sam_lines over text[:n_bytes] -> the five words of ``status`` on the host: the round's one wait"""
        import ctypes as C
        _lib.check(self._lib.besst_dev_sam_lines(C.c_void_p(main.cuda_stream), C.c_void_p(text.data_ptr()), int(n_bytes),
                                                 1 if want_header_end else 0, int(count_upto), C.c_void_p(status.data_ptr())),
                   'besst_dev_sam_lines')
        return status.cpu().tolist()

    def _long_line(self, at, chunk):
        return SamError('%s: the line at byte %d of the inflated text is longer than chunk_bytes = %d; raise chunk_bytes'
                        % (self.path, at, chunk), at, None, 'line longer than a chunk')

    def _host_round(self, torch, dev, taken, text):
        """The blocks of a round inflated by zlib and laid where the device would have put them."""
        with open(self.path, 'rb') as fh:
            for tab, a, b, place in taken:
                parts = []
                for k in range(a, b):
                    fh.seek(int(tab['payload_at'][k]))
                    at = int(tab['starts'][k])
                    try:
                        raw = zlib.decompress(fh.read(int(tab['src_len'][k])), -15)
                    except zlib.error as exc:
                        raise self._compressed_error('the BGZF block at byte %d of the compressed SAM file does not inflate: %s'
                                                     % (at, exc), at)
                    if len(raw) != int(tab['isize'][k]) or (zlib.crc32(raw) & 0xffffffff) != int(tab['crc'][k]):
                        raise self._compressed_error('the BGZF block at byte %d of the compressed SAM file is damaged: its '
                                                     'inflated bytes are not those of its CRC-32 and ISIZE' % at, at)
                    parts.append(raw)
                raw = b''.join(parts)
                if raw:
                    text[place:place + len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        torch.cuda.current_stream(dev).synchronize()

    # ---- gzip with gzip_on_gpu: the text is inflated into HBM whole and parsed in place -----------------------------------
    def _parse_resident(self, device, device_index, torch, dev, text, n):
        with torch.cuda.device(dev):
            # the header is fetched back from the front of the text
            header, h_bytes, window, done = [], 0, 1 << 20, False
            while not done and h_bytes < n:
                front = text[h_bytes:min(n, h_bytes + window)].cpu().numpy().tobytes()
                at_end, at = h_bytes + len(front) == n, 0
                while at < len(front):
                    if front[at:at + 1] != b'@':
                        done = True
                        break
                    nl = front.find(b'\n', at)
                    if nl < 0 and not at_end:
                        break                                    # the line goes on behind the window
                    line = front[at:] if nl < 0 else front[at:nl + 1]
                    header.append(line)
                    at += len(line)
                h_bytes += at
                if at == 0 and not done:
                    window *= 4                                  # a header line longer than the window
            self._open_context(device, device_index, header)
            body = n - h_bytes
            if body == 0:
                return
            if h_bytes % 16:                                     # the parser wants its text 16-byte aligned: the records move
                step = 32 << 20                                  # down over the header, front to back through a bounce buffer
                tmp = torch.empty(min(step, body), dtype=torch.uint8, device=dev)
                for lo in range(0, body, step):
                    k = min(step, body - lo)
                    tmp[:k].copy_(text[h_bytes + lo:h_bytes + lo + k])
                    text[lo:lo + k].copy_(tmp[:k])
                text[body:body + min(16, h_bytes)].zero_()
                base = text.data_ptr()
            else:
                base = text.data_ptr() + h_bytes
            info = self._push(torch.cuda.current_stream(dev).cuda_stream, base, body, h_bytes)
            if info[2] >= 0:
                rel = int(info[2]) - h_bytes
                moved = h_bytes if h_bytes % 16 else 0
                lo = h_bytes - moved
                line = len(header) + 1 + int((text[lo:lo + rel] == 10).sum().item())
                raise _sam_error(self.path, info, line, True)
            del text

    def __len__(self):
        return self._n

    def layout_state(self):
        """GraphContext.layout_state(): after a SAM ingest the three watermarks stand at 0 - the planes and the candidate
        side stream are made by the first build."""
        return self.ctx.layout_state()

    def report(self, isize_bins=32768):
        """The report of the file (GraphContext.library_report, besst_amd.report) with the header's names and lengths."""
        rep = self.ctx.library_report(isize_bins)
        rep.references, rep.lengths = list(self.references), [int(x) for x in self.lengths]
        return rep

    def close(self):
        if self.ctx is not None:
            self.ctx.close()


def _split_lines(data):
    """bytes -> its lines with their '\\n' (only '\\n' ends a line); a last line without one is a line"""
    lines = data.split(b'\n')
    last = lines.pop()
    return [line + b'\n' for line in lines] + ([last] if last else [])


class _MemberStream(object):
    """``readinto`` over the inflated bytes of the gzip members of an open file (GenerateOutput._gzip_members: zlib on the
    host, a piece at a time) behind ``prefix``, for ResidentSam._stream_lines; ``header_lines`` takes the leading '@' lines."""

    def __init__(self, fh, base=0, prefix=b''):
        from . import GenerateOutput as GO
        self._pieces = GO._gzip_members(fh, base=base)
        self._buf, self._at = bytes(prefix), 0

    def _more(self):
        while self._at >= len(self._buf):
            piece = next(self._pieces, None)
            if piece is None:
                return False
            self._buf, self._at = piece, 0
        return True

    def readinto(self, view):
        got = 0
        while got < len(view) and self._more():
            k = min(len(view) - got, len(self._buf) - self._at)
            view[got:got + k] = memoryview(self._buf)[self._at:self._at + k]
            got, self._at = got + k, self._at + k
        return got

    def header_lines(self):
        """-> (the leading run of '@' lines, their bytes); the stream stands behind them"""
        lines, size = [], 0
        while self._more() and self._buf[self._at] == 64:
            parts = []
            while self._more():
                nl = self._buf.find(b'\n', self._at)
                stop = len(self._buf) if nl < 0 else nl + 1
                parts.append(self._buf[self._at:stop])
                self._at = stop
                if nl >= 0:
                    break
            lines.append(b''.join(parts))
            size += len(lines[-1])
        return lines, size


def _read_full(fh, view):
    """readinto until the view is full or the file ends -> bytes read"""
    got = 0
    while got < len(view):
        k = fh.readinto(view[got:])
        if not k:
            break
        got += k
    return got


def _last_line_end(view, have):
    """The offset behind the last '\\n' of view[:have] (0: none), looked for from the end in windows."""
    hi = have
    while hi > 0:
        lo = max(0, hi - (1 << 16))
        at = bytes(view[lo:hi]).rfind(b'\n')
        if at >= 0:
            return lo + at + 1
        hi = lo
    return 0


def sniff_format(path):
    """'bam' or 'sam', by content: a file that begins with the gzip magic and whose first member's first bytes (zlib on
    the host, the first 64 KiB of the file) inflate to ``BAM\\1`` is a BAM - and so is one whose first member cannot be
    inflated, so that every error of the BAM reader stays what it is; gzip around any other text, and a file without the
    gzip magic, is SAM."""
    with open(path, 'rb') as fh:
        front = fh.read(65536)
    if front[:2] != GZIP_MAGIC:
        return 'sam'
    first, data = b'', front
    try:
        while len(first) < 4 and data:                           # (an empty member in front - a BGZF EOF block - is passed over)
            d = zlib.decompressobj(31)
            first += d.decompress(data, 1 << 20)                 # (as far as the 64 KiB go: damage there is the BAM reader's to name)
            if not d.eof:
                break
            data = d.unused_data
    except zlib.error:
        return 'bam'
    if len(first) < 4 and not d.eof:
        return 'bam'                                             # the member ends early: the BAM reader says so
    return 'bam' if first[:4] == b'BAM\1' else 'sam'


def reader_class(path):
    """The class open_bam uses for ``path`` outside a process group (no device is touched)."""
    return ResidentBam if sniff_format(path) == 'bam' else ResidentSam


SHARDED_SAM_MESSAGE = ('%s is SAM text: under a process group the sharded input is BAM (every rank reads its slice of the BGZF '
                       'blocks); convert the file to BAM or run on one GPU')


def open_bam(path, threads=None, **kw):
    """What a caller of the two entry points opens in place of ``pysam.Samfile(path, 'rb')`` (runBESST:162): a ResidentBam,
    a ResidentSam where the file is SAM text (plain, BGZF or gzip: sniff_format), or - under a process group for which
    sharding has been switched on (sharded.enable() / BESST_SHARDED=1: torchrun, one process per GPU) - this rank's
    ShardedBam.  A SAM file under a process group is refused on every rank alike, before any collective."""
    from . import sharded
    cls = reader_class(path)
    if sharded.active_group() is not None:
        if cls is ResidentSam:
            raise ValueError(SHARDED_SAM_MESSAGE % path)
        return ShardedBam(path, group=sharded.PROCESS_GROUP, threads=threads,
                          **{k: v for k, v in kw.items() if k in ('device_index', 'chunk_blocks')})
    if cls is ResidentSam:
        return ResidentSam(path, **{k: v for k, v in kw.items() if k in ('device_index', 'chunk_bytes', 'tile_bytes', 'gzip_on_gpu')})
    return ResidentBam(path, threads=threads, **{k: v for k, v in kw.items() if k != 'gzip_on_gpu'})


def inflate_bgzf_device(data, device_index=0, out_cap=None):
    """Test hook: the BGZF blocks of ``data`` (bytes) inflated by the GPU kernel, concatenated."""
    import ctypes as C
    lib = _lib.load()
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(out_cap if out_cap is not None else max(1, 66 * len(data)), dtype=np.uint8)
    n = C.c_size_t(0)
    _lib.check(lib.besst_bgzf_inflate_device(int(device_index), _lib.ptr(src), len(data), _lib.ptr(out), out.size, C.byref(n)),
               'bgzf_inflate_device')
    return out[:n.value].tobytes()


def write_bam(path, batch, threads=None, level=1, realistic=False):
    """Test / bench scaffolding (besst_bam_write_records): the batch as a BAM file in htslib's block layout.  realistic:
    pseudo-random bases and slowly changing qualities instead of constant bytes (the file compresses ~3 x, not ~13 x)."""
    if realistic:
        level = int(level) | 16
    import ctypes as C
    lib = _lib.load()
    names = (C.c_char_p * len(batch.references))(*[n.encode() for n in batch.references])
    lengths = np.ascontiguousarray(batch.lengths, dtype=np.int32)
    rlen = batch.rlen if batch.rlen is not None else batch.qlen
    cols = [_lib.as_col(batch.tid, np.int32), _lib.as_col(batch.mtid, np.int32), _lib.as_col(batch.pos, np.int32),
            _lib.as_col(batch.mpos, np.int32), _lib.as_col(batch.tlen, np.int32), _lib.as_col(batch.flag, np.uint16),
            _lib.as_col(batch.mapq, np.uint8), _lib.as_col(batch.qlen, np.uint16), _lib.as_col(rlen, np.int32)]
    _lib.check(lib.besst_bam_write_records(os.fsencode(path), len(batch.references), names, _lib.ptr(lengths), len(batch),
                                           *[_lib.ptr(c) for c in cols], int(threads or reader_threads()),
                                           int(level)), 'bam_write_records')


def read_bam(path, threads=None, chunk_records=8_000_000):
    lib = _lib.load()
    threads = threads or reader_threads()
    handle = lib.besst_bam_open(os.fsencode(path), int(threads))
    if not handle:
        raise IOError('cannot read BAM %s: %s' % (path, _lib.last_error()))
    try:
        names, lengths = _header(lib, handle)
        spec = (('tid', np.int32), ('mtid', np.int32), ('pos', np.int32), ('mpos', np.int32), ('tlen', np.int32),
                ('flag', np.uint16), ('mapq', np.uint8), ('qlen', np.uint16), ('rlen', np.int32), ('alen', np.int32))
        parts = {k: [] for k, _ in spec}
        while True:
            bufs = [np.empty(chunk_records, dtype=dt) for _, dt in spec]
            got = lib.besst_bam_read_records(handle, chunk_records, *[_lib.ptr(b) for b in bufs])
            if got < 0:
                raise IOError('error while reading %s: %s' % (path, _lib.last_error()))
            if got == 0:
                break
            for (k, _), b in zip(spec, bufs):
                parts[k].append(b[:got])
        cols = {k: (np.concatenate(v) if v else np.empty(0, dtype=dt)) for (k, dt), v in zip(spec, parts.values())}
        clamped = lib.besst_bam_clamped_records(handle)
        if clamped > 0:
            import warnings
            warnings.warn('%s: %d record(s) align more than 65535 query bases; their qlen (the coverage numerator of '
                          'CreateGraph.py:138-139) is stored as 65535' % (path, clamped))
    finally:
        lib.besst_bam_close(handle)
    return RecordBatch(names, lengths, **cols)
