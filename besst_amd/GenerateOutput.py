"""Output of the scaffolding result, and the four helpers that the hot path calls from inside CreateGraph.PE.

The helpers (reference: GenerateOutput.py:47-85, called at CreateGraph.py:432,803,1012-1013) matter for parity because
they DELETE the removed contigs from the caller's dicts.

``WriteToF`` / ``PrintOutput`` (reference :88-227) write ``Scaffolds-pass<n>.fa``, ``info-pass<n>.agp`` and
``info-pass<n>.gff``.  The sequence work is done on the device (csrc/emit.hip): the contigs lie in a
:class:`SequenceStore` in HBM for the whole run, ``seq_overlap_kernel`` finds the overlaps of the junctions that may
merge, the host turns placements + overlaps into a piece table with numpy, and ``emit_kernel`` gathers the FASTA bytes
(copy / reverse-complement / 'N' fill).
With ``param.outputs_bgzf`` the bytes are compressed on the device first (csrc/bgzf_deflate.hip) and the file is
``Scaffolds-pass<n>.fa.gz``, a BGZF file: only the compressed bytes cross PCIe.
AGP and GFF are plain text from names, positions and gaps: on the host by default, and with ``param.outputs_on_gpu`` formatted
on the device from flat columns and the store's name pool (csrc/emit_text.hip).  A store with ``batch_fasta`` set also
writes ``repeats.fa`` / ``low_coverage_contigs.fa`` from the pool with one kernel instead of one fetch per contig.
Every file that is produced on the device is a byte source (``total`` bytes, ``emit`` of a range, ``check`` after the last
range: :class:`ScaffoldEmitter`, ``_TextEmitter.file``, ``wrapped_fasta_source``) and reaches the host through one
pipeline, :func:`write_chunks`: chunks cut by :func:`chunk_plan` go through two slots of device and pinned buffers, the
copy and the file write of chunk c running while the kernels of chunk c + 1 do.
``SequenceStore.from_fasta`` fills the store from the contig
FASTA itself (csrc/fasta.hip: the file's bytes are parsed in HBM by the rules of runBESST:45-74); ``C_dict`` then holds
:class:`SequenceRef` handles instead of strings.  A file that begins with the gzip magic is inflated first: a BGZF file
(what ``--bgzf_outputs`` and ``bgzip`` write) on the device, block by block at its place in the text
(:func:`_upload_bgzf_file`); any other gzip file by zlib on the host (:func:`_upload_gzip_host`) -
or, with ``gzip_on_gpu``, a file of one or of several gzip members on the device as well (:func:`_upload_gzip_device`, csrc/gzip_stream.hip).  Like the rest of the package there is no CPU path: without
the library or a GPU these calls raise :class:`besst_amd._lib.BesstDeviceError`.
"""
from __future__ import print_function

import ctypes as _C
import io
import os
import time
import warnings
import zlib

import numpy as np

from . import _lib
from ._lib import BesstDeviceError


def _write_fasta(handle, name, sequence):
    print('>' + name, file=handle)
    sequence = sequence or ''
    for i in range(0, len(sequence), 60):
        print(sequence[i:i + 60], file=handle)


def _forget(cont_obj, Contigs, small_contigs):
    try:
        del Contigs[cont_obj.name]
    except KeyError:
        del small_contigs[cont_obj.name]


def _write_from_pool(cont_objs, path):
    """The contigs as wrapped FASTA straight from the sequence pool (csrc/emit_text.hip: wrap_fasta_kernel) if every
    sequence is a :class:`SequenceRef` of one store that has ``batch_fasta`` set and knows the contig by its name.
    -> False: nothing was written, the caller's own loop has to."""
    store, rows = None, []
    for cont_obj in cont_objs:
        seq = cont_obj.sequence
        if not isinstance(seq, SequenceRef) or (store is not None and seq.store is not store):
            return False
        store = seq.store
        if not store.batch_fasta or store.name_of(seq.row) != cont_obj.name:
            return False
        rows.append(seq.row)
    if store is None:
        return False
    try:
        store.name_pool()
    except UnicodeEncodeError:
        return False
    write_wrapped_fasta(store, rows, path)
    return True


def _print_out_fasta(cont_objs, Contigs, output_dest, small_contigs, file_name):
    """reference :47-53, 68-74: the contigs as wrapped FASTA into ``file_name`` (no ``output_dest``: no file), every one
    of them deleted from the caller's dicts."""
    path = output_dest + '/' + file_name if output_dest else None
    handle = open(path, 'w') if path and not _write_from_pool(cont_objs, path) else None
    for cont_obj in cont_objs:
        if handle:
            _write_fasta(handle, cont_obj.name, cont_obj.sequence)
        _forget(cont_obj, Contigs, small_contigs)
    if handle:
        handle.close()
    return ()


def PrintOutRepeats(Repeats, Contigs, output_dest, small_contigs):
    return _print_out_fasta(Repeats, Contigs, output_dest, small_contigs, 'repeats.fa')


def repeat_contigs_logger(Repeats, Contigs, output_dest, small_contigs, param):
    if not output_dest:
        return
    with open(output_dest + '/repeats_log.tsv', 'w') as handle:
        print('contig_accession\tlength\tcoverage\tcov/mean_cov(exp number of placements)\tlib_mean\tplacable',
              file=handle)
        for cont_obj in sorted(Repeats, key=lambda c: c.coverage, reverse=True):
            placable = 'Yes' if param.mean_ins_size > cont_obj.length else 'No'
            print('{0}\t{1}\t{2}\t{3}\t{4}\t{5}'.format(
                cont_obj.name, cont_obj.length, round(cont_obj.coverage, 1),
                round(cont_obj.coverage / param.mean_coverage, 0), round(param.mean_ins_size, 0), placable),
                file=handle)


def PrintOut_low_cowerage_contigs(low_coverage_contigs, Contigs, output_dest, small_contigs):
    return _print_out_fasta(low_coverage_contigs, Contigs, output_dest, small_contigs, 'low_coverage_contigs.fa')


def ChangeToSmallContigs(Contigs, list_of_contigs, small_contigs):
    for cont_obj in list_of_contigs:
        del Contigs[cont_obj.name]
        small_contigs[cont_obj.name] = cont_obj
    return ()


# ---- the scaffolds themselves: FASTA / AGP / GFF (reference GenerateOutput.py:88-227) -----------------------------------
MAX_CONTIG_OVERLAP_LIMIT = 4096          # include/besst_amd.h: BESST_MAX_CONTIG_OVERLAP
EMIT_PAD = 32                            # include/besst_amd.h: BESST_EMIT_PAD
PIECE_COPY, PIECE_REVCOMP, PIECE_FILL_N, PIECE_LITERAL = 0, 1, 2, 3
MIN_MERGE_OVERLAP = 20                   # reference :140
CHUNK_BYTES = 256 << 20                  # PrintOutput produces the FASTA in chunks of this size
NO_ERROR = 0xFFFFFFFFFFFFFFFF
TEXT_THREADS = 256                       # include/besst_amd.h: BESST_TEXT_THREADS (contigs per workgroup, flags / measure)
TEXT_SCAN_CHUNK = 4096                   # include/besst_amd.h: BESST_TEXT_SCAN_CHUNK (entries per turn of the scans)
TEXT_TILE_BYTES = 16384                  # include/besst_amd.h: BESST_TEXT_TILE_BYTES (file bytes per workgroup, AGP / GFF)
WRAP_TILE_BYTES = 16384                  # include/besst_amd.h: BESST_WRAP_TILE_BYTES (file bytes per workgroup, wrapped FASTA)
TEXT_AGP, TEXT_GFF = 0, 1
TEXT_INFO_WORDS = 3                      # include/besst_amd.h: BESST_TEXT_INFO_WORDS
TEXT_LIMIT = 1 << 62                     # positions and lengths of this magnitude or more are left to the host writer
FASTA_LINE = 60                          # bases per line of repeats.fa / low_coverage_contigs.fa
BGZF_BLOCK_PAYLOAD = 65280               # include/besst_amd.h: BESST_BGZF_BLOCK_PAYLOAD (htslib's); read where it is used
BGZF_EOF = bytes(bytearray([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
last_timings = {}                        # PrintOutput's wall-time split of its latest call (seconds)


def WriteToF(F, Contigs, list_of_contigs):
    info_list = []
    for cont_obj in list_of_contigs:
        info_list.append((cont_obj.name, cont_obj.direction, cont_obj.position, cont_obj.length, cont_obj.sequence))
        if cont_obj.position < 0:
            print('Write to F: Position is negative!', cont_obj.position, cont_obj.name, cont_obj.direction)
    F.append(info_list)
    return F


def pack_sequences(sequences):
    """-> (pool uint8, offsets int64, lengths int32): the sequences end to end, one byte per base, as given."""
    parts = []
    for seq in sequences:
        if isinstance(seq, str):
            try:
                seq = seq.encode('ascii')
            except UnicodeEncodeError:
                raise ValueError('contig sequences must be ASCII')
        elif seq is None:
            seq = b''
        else:
            seq = bytes(seq)
            if seq.translate(None, _ASCII):
                raise ValueError('contig sequences must be ASCII')
        parts.append(seq)
    lengths = np.fromiter((len(p) for p in parts), dtype=np.int64, count=len(parts))
    if len(parts) and int(lengths.max()) >= 1 << 31:
        raise ValueError('a contig of 2^31 bases or more')
    offsets = np.zeros(len(parts), dtype=np.int64)
    if len(parts) > 1:
        np.cumsum(lengths[:-1], out=offsets[1:])
    pool = np.frombuffer(b''.join(parts), dtype=np.uint8)
    return pool, offsets, lengths.astype(np.int32)


_ASCII = bytes(range(128))


def _torch_device(device):
    try:
        import torch
    except ImportError as exc:
        raise BesstDeviceError('scaffold output needs torch for ROCm: %s' % exc)
    _lib.load()
    if not torch.cuda.is_available():
        raise BesstDeviceError('scaffold output needs a GPU (besst_amd has no CPU fallback)')
    return torch, torch.device('cuda', int(device))


def _padded_upload(torch, dev, host_bytes):
    """uint8 tensor with EMIT_PAD zero bytes on either side of the data -> (tensor, pointer of the data)."""
    n = int(host_bytes.shape[0])
    t = torch.zeros(n + 2 * EMIT_PAD, dtype=torch.uint8, device=dev)
    if n:
        with warnings.catch_warnings():                          # a read-only view of a bytes object: it is only read
            warnings.simplefilter('ignore', UserWarning)
            t[EMIT_PAD:EMIT_PAD + n].copy_(torch.from_numpy(host_bytes))
    return t, t.data_ptr() + EMIT_PAD


class SequenceStore(object):
    """The contig sequences of a run in HBM: uploaded once, read by every pass's output (only placements change between
    libraries).  One byte per base - case and IUPAC codes survive.

    ``batch_fasta``: PrintOutRepeats / PrintOut_low_cowerage_contigs write their files from the pool in one go."""
    batch_fasta = False
    _names = _name_off = _name_at = None

    def __init__(self, names, sequences, device=0):
        names = self._name_list = list(names)
        pool, self.offsets, self.lengths = pack_sequences(sequences)
        if len(names) != len(self.offsets):
            raise ValueError('need one name per sequence')
        self.index = {name: i for i, name in enumerate(names)}
        self.pool_bytes = int(pool.shape[0])
        torch, dev = _torch_device(device)
        self.device = dev
        self._pool, self.pool_ptr = _padded_upload(torch, dev, pool)
        self._off = torch.from_numpy(self.offsets).to(dev)
        self._len = torch.from_numpy(self.lengths).to(dev)

    @classmethod
    def from_contigs(cls, Contigs, small_contigs, device=0):
        objs = list(Contigs.values()) + list(small_contigs.values())
        return cls([c.name for c in objs], [c.sequence for c in objs], device=device)

    inflate = None
    inflate_stats = None

    @classmethod
    def from_fasta(cls, path, device=0, tile_bytes=None, blocks_per_launch=None, gzip_on_gpu=False, gzip_chunk_bytes=None):
        """The store of a contig FASTA, parsed on the device (csrc/fasta.hip) with the rules of the reference's
        ReadInContigseqs (runBESST:45-74): one row per header line in file order (``names``); ``index[name]`` is the row
        of the name's last occurrence.  ValueError: a byte outside ASCII, a header without a name, a contig of 2^31 bases
        or more.

        A file whose first two bytes are the gzip magic (its name does not matter) is inflated on the way: on the device
        if it is BGZF from its first byte to its last, at most ``blocks_per_launch`` blocks (BLOCKS_PER_LAUNCH) per launch,
        by zlib on the host if it is any other gzip file or holds a block the device kernel does not take.  ``inflate``
        of the store says which: None, 'device' or 'host'.  FastaError with the COMPRESSED offset of the block or member
        at fault: a CRC-32 or ISIZE that is not the inflated bytes', a file that ends inside a member, bytes behind the
        last member that are none, data zlib does not inflate.  The parser's own errors then count bytes of the
        inflated text.

        ``gzip_on_gpu``: a gzip file that is not BGZF - ``gzip``'s own output, one member or a series of them - is inflated
        on the device too (:func:`_upload_gzip_device`: block and member starts found by probing, chunks of
        ``gzip_chunk_bytes`` compressed bytes decoded against windows that are resolved afterwards); ``inflate`` is then
        'device_gzip'.  Whatever the device does not take or finds damaged - an odd header, more member candidates than
        its list holds, DEFLATE data, ISIZE or a CRC-32 that is wrong, memory that runs out - is read on the host exactly as
        without the flag, errors included; ``inflate`` is 'host' then and ``inflate_stats['status']`` names the device's
        reason.  ``inflate_stats``: chunks, candidates (chunks in which a block start was found), live (segments that were
        decoded side by side), text_bytes, members, member_candidates (offsets that read like a member's start), status
        (None: the device's gzip path was not tried), and bad_member / bad_member_offset where the device names one.  ``gzip_chunk_bytes``: a multiple of 16 in 256..2^24 (GZIP_CHUNK_BYTES)."""
        chunk = int(GZIP_CHUNK_BYTES if gzip_chunk_bytes is None else gzip_chunk_bytes)
        if chunk < 256 or chunk > (1 << 24) or chunk % 16:
            raise ValueError('gzip_chunk_bytes must be a multiple of 16 in 256..2^24')
        torch, dev = _torch_device(device)
        stats = dict(chunks=0, candidates=0, live=0, text_bytes=0, status=None)
        with open(path, 'rb') as fh:
            gz = fh.read(2) == GZIP_MAGIC
        with torch.cuda.device(dev):
            if gz:
                try:
                    text, n, inflate = _upload_gzip_file(torch, dev, path, blocks_per_launch, chunk if gzip_on_gpu else None, stats)
                except FastaError as exc:
                    exc.inflate_stats = stats                    # (what the device made of the file before the host read it)
                    raise
            else:
                (text, n), inflate = _upload_file(torch, dev, path), None
            try:
                parsed = parse_fasta_text(text, n, tile_bytes)
            except FastaError as exc:
                if inflate is not None:
                    exc = FastaError('%s (bytes of the inflated text: the file is compressed)' % exc, exc.offset)
                exc.inflate_stats = stats
                raise exc
            del text
        self = cls.__new__(cls)
        self.device = dev
        self.inflate, self.inflate_stats = inflate, stats
        self._pool, self.pool_ptr, self.pool_bytes = parsed['pool'], parsed['pool'].data_ptr() + EMIT_PAD, parsed['pool_bytes']
        self._off, self._len = parsed['ctg_off'], parsed['ctg_len']
        self.offsets, self.lengths = self._off.cpu().numpy(), self._len.cpu().numpy()
        self._names, self._name_off = parsed['names'], parsed['name_off']
        self._name_at = self._name_off.cpu().numpy()
        blob, at = self._names.cpu().numpy().tobytes().decode('ascii'), self._name_at.tolist()
        self.names = [blob[a:b] for a, b in zip(at[:-1], at[1:])]
        self.index = {name: i for i, name in enumerate(self.names)}
        return self

    def name_of(self, row):
        names = getattr(self, 'names', None)
        return (self._name_list if names is None else names)[row]

    def set_names(self, names):
        """Other names for the rows (PrintOutput's own store: the contig names of F); the pool is built on demand."""
        self._name_list = list(names)
        self._names = self._name_off = self._name_at = None

    def name_pool(self):
        """The names of the rows end to end on the device -> (uint8 tensor, int64 offsets tensor of len(self) + 1
        entries, the same offsets as numpy).  A from_fasta store keeps what the parser left; a store built from Python
        strings uploads the blob at the first call.  UnicodeEncodeError: a name is not ASCII."""
        if self._names is None:
            import torch
            parts = [str(n).encode('ascii') for n in self._name_list]
            at = np.zeros(len(parts) + 1, dtype=np.int64)
            np.cumsum(np.fromiter((len(b) for b in parts), dtype=np.int64, count=len(parts)), out=at[1:])
            blob = np.frombuffer(b''.join(parts) or b'\0', dtype=np.uint8)
            with warnings.catch_warnings():                      # a read-only view of a bytes object: it is only read
                warnings.simplefilter('ignore', UserWarning)
                self._names = torch.from_numpy(blob).to(self.device)
            self._name_off, self._name_at = torch.from_numpy(at).to(self.device), at
        return self._names, self._name_off, self._name_at

    def fetch(self, row):
        """The bytes of contig ``row``, copied back from the pool."""
        off, length = int(self.offsets[row]), int(self.lengths[row])
        return self._pool[EMIT_PAD + off:EMIT_PAD + off + length].cpu().numpy().tobytes()

    def contig_dict(self, filter_length=None, Information=None):
        """name -> SequenceRef in the reference's dictionary order (a name that occurs twice: the place of its first
        occurrence, the sequence of its last), the way CreateGraph.PE takes ``C_dict``.  ``filter_length``: -filter_contigs
        (runBESST:67-73) - shorter contigs are left out; their bases stay in the pool, unused.  With ``Information`` the
        reference's two lines are printed to it."""
        names = getattr(self, 'names', None)
        if names is None:
            names = sorted(self.index, key=self.index.get)
        contigs = {}
        for name in names:
            if name not in contigs:
                row = self.index[name]
                contigs[name] = SequenceRef(self, row, int(self.lengths[row]))
        return filter_contigs(contigs, filter_length, Information)

    def __len__(self):
        return len(self.offsets)

    def byte_at(self, pool_offset):
        return int(self._pool[EMIT_PAD + int(pool_offset)].item())

    def report(self, rows=None, min_gap=1):
        """The census of the contigs (seqreport.census_store): bases by class, lower case, runs of 'N', per row."""
        from . import seqreport
        return seqreport.census_store(self, rows, min_gap)

    def close(self):
        self._pool = self._off = self._len = self._names = self._name_off = None
        self.pool_ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SequenceRef(object):
    """A contig's sequence that stays in the store: what InitializeObjects and the repeat / low-coverage FASTA writers ask
    of a sequence (len, truth, slices, str) without the bases in host memory.  The first use that needs bases fetches them
    once."""
    __slots__ = ('store', 'row', 'length', '_bytes')

    def __init__(self, store, row, length):
        self.store, self.row, self.length, self._bytes = store, row, length, None

    def __len__(self):
        return self.length

    def __bool__(self):
        return self.length > 0

    def _fetched(self):
        if self._bytes is None:
            self._bytes = self.store.fetch(self.row)
        return self._bytes

    def __getitem__(self, key):
        got = self._fetched()[key]
        return chr(got) if isinstance(got, int) else got.decode('ascii')

    def __str__(self):
        return self._fetched().decode('ascii')


def filter_contigs(contigs, filter_length, Information=None):
    """-filter_contigs as runBESST:65-73 meant it (on Python 3 the reference raises RuntimeError here: it deletes from the
    dict whose keys it walks): contigs shorter than ``filter_length`` leave the dict.  The two lines go to ``Information``
    in the reference's words."""
    if Information is not None:
        print('Initial number of contigs: {}. '.format(len(contigs)), file=Information)
    if filter_length:
        short = [name for name, seq in contigs.items() if len(seq) < filter_length]
        for name in short:
            del contigs[name]
        if Information is not None:
            print('Number of contigs discarded from further analysis (with -filter_contigs set to {0}): {1}'.format(
                filter_length, len(short)), file=Information)
    return contigs


class FastaError(ValueError):
    """The contig FASTA cannot be read; ``offset``: the byte of the file at fault.  ``inflate_stats``: from_fasta's, where a
    compressed file was at fault."""
    inflate_stats = None

    def __init__(self, message, offset):
        ValueError.__init__(self, message)
        self.offset = offset


UPLOAD_CHUNK = 32 << 20                  # from_fasta reads the file through two pinned buffers of this size
FASTA_INFO_WORDS = 6                     # include/besst_amd.h: BESST_FASTA_INFO_WORDS


def _upload_file(torch, dev, path):
    """file -> pinned buffer -> HBM, two buffers and a side stream: the read of chunk c + 1 runs while chunk c is copied.
    -> (uint8 tensor of the file's bytes followed by EMIT_PAD zero bytes, number of bytes)"""
    with open(path, 'rb', buffering=0) as fh:
        n = os.fstat(fh.fileno()).st_size
        text = torch.empty(n + EMIT_PAD, dtype=torch.uint8, device=dev)
        text[n:].zero_()
        size = max(1, min(UPLOAD_CHUNK, n))
        h_buf = [torch.empty(size, dtype=torch.uint8).pin_memory() for _ in range(2)]
        views = [memoryview(b.numpy()) for b in h_buf]
        done = [None, None]
        copy = torch.cuda.Stream(dev)
        copy.wait_stream(torch.cuda.current_stream(dev))
        at, i = 0, 0
        while at < n:
            slot = i % 2
            if done[slot] is not None:
                done[slot].synchronize()                        # the buffer's last copy has left it
            got = fh.readinto(views[slot][:min(size, n - at)])
            if not got:
                raise IOError('%s ended %d bytes early' % (path, n - at))
            with torch.cuda.stream(copy):
                text[at:at + got].copy_(h_buf[slot][:got], non_blocking=True)
                done[slot] = torch.cuda.Event()
                done[slot].record(copy)
            at += got
            i += 1
        torch.cuda.current_stream(dev).wait_stream(copy)
        copy.synchronize()                                       # the pinned buffers are let go here
    return text, n


GZIP_MAGIC = b'\x1f\x8b'
BLOCKS_PER_LAUNCH = 4096                 # BGZF blocks per launch of the inflate: four bytes of symbol workspace per inflated byte
BGZF_WINDOW_BLOCKS = 1 << 16             # block descriptors a window's buffers hold (a window of more blocks is cut there)
BGZF_DESC_BYTES = 24                     # include/besst_amd.h: sizeof(besst_bgzf_block)
BGZF_MAX_BLOCK = 65536                   # a BGZF block's size in the file at most: the smallest window that holds a whole block
BGZF_COMP_PAD = 4096                     # readable bytes the inflate wants behind the last payload
BGZF_BAD_SIZE, BGZF_BAD_CRC = 9, 10      # include/besst_amd.h: BESST_BGZF_BAD_SIZE, BESST_BGZF_BAD_CRC


def bgzf_walk(path, max_blocks=-1):
    """The file as a chain of BGZF blocks (besst_bgzf_walk) -> (blocks, sum of their ISIZE, offset of the first byte that
    is no whole BGZF block, size of the file); at most ``max_blocks`` blocks (< 0: all)."""
    lib = _lib.load()
    size = os.path.getsize(path)
    n, inflated, end = _C.c_int64(0), _C.c_int64(0), _C.c_size_t(0)
    if size:
        data = np.memmap(path, dtype=np.uint8, mode='r')
        _lib.check(lib.besst_bgzf_walk(_C.c_void_p(data.ctypes.data), int(data.shape[0]), int(max_blocks), _C.byref(n),
                                       _C.byref(inflated), _C.byref(end)), 'besst_bgzf_walk')
        size = int(data.shape[0])
        del data
    return n.value, inflated.value, end.value, size


def _first_bad(word):
    """The device's word of the first bad block -> (block, reason), or None"""
    bad = int(word.item()) & NO_ERROR
    return None if bad == NO_ERROR else (bad >> 8, bad & 0xff)


def _upload_gzip_file(torch, dev, path, blocks_per_launch=None, gzip_chunk_bytes=None, stats=None):
    """A file that begins with the gzip magic -> (text, n, 'device', 'device_gzip' or 'host'), text as _upload_file leaves
    it.  ``gzip_chunk_bytes``: a file that is not BGZF is tried on the device first (``stats``: what that left)."""
    n_blocks, total, end, size = bgzf_walk(path)
    if end == size:
        got = _upload_bgzf_file(torch, dev, path, n_blocks, total, blocks_per_launch)
        if got is not None:
            return got[0], got[1], 'device'
    elif gzip_chunk_bytes:
        got = _upload_gzip_device(torch, dev, path, gzip_chunk_bytes, {} if stats is None else stats)
        if got is not None:
            return got[0], got[1], 'device_gzip'
    text, n = _upload_gzip_host(torch, dev, path)
    return text, n, 'host'


def _upload_bgzf_file(torch, dev, path, n_blocks, total, blocks_per_launch=None):
    """The sibling of _upload_file for a file that is ``n_blocks`` BGZF blocks of ``total`` inflated bytes and nothing else:
    the file goes through two pinned buffers in windows, a window's block descriptors (besst_bgzf_scan_chunk) and
    compressed bytes go up on the side stream, and the inflate of window c (besst_dev_bgzf_inflate: inflate, CRC-32,
    first bad block) is enqueued while window c + 1 is read.  A block the window's end cuts is carried into the next
    window.  Every block lands at its final place in the one text buffer; one synchronisation behind the last window
    reads the first bad block.  -> (text, total), or None: the device kernel does not take a block's DEFLATE data (the
    caller reads the file on the host).  FastaError: a block's CRC-32 or ISIZE is not its inflated bytes'."""
    lib = _lib.load()
    p = _C.c_void_p
    per_launch = max(1, min(int(blocks_per_launch or BLOCKS_PER_LAUNCH), n_blocks))
    ws_bytes = lib.besst_dev_bgzf_inflate_workspace_bytes(per_launch, min(per_launch * 65536, total))
    if not ws_bytes:
        raise ValueError('blocks_per_launch must lie in 1..2^24')
    main = torch.cuda.current_stream(dev)
    text = torch.empty(total + EMIT_PAD, dtype=torch.uint8, device=dev)
    text[total:].zero_()
    first_bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with open(path, 'rb', buffering=0) as fh:
        size = os.fstat(fh.fileno()).st_size
        cap = max(1, min(size, max(int(UPLOAD_CHUNK), BGZF_MAX_BLOCK)))   # a window: carried bytes + new ones, a whole block at least
        desc_cap = max(2, min(BGZF_WINDOW_BLOCKS, n_blocks + (n_blocks & 1)))
        desc_bytes = desc_cap * BGZF_DESC_BYTES                  # (a multiple of 16: the payloads' words stay aligned)
        h_buf = [torch.empty(desc_bytes + cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        d_buf = [torch.zeros(desc_bytes + cap + BGZF_COMP_PAD, dtype=torch.uint8, device=dev) for _ in range(2)]
        views = [memoryview(b.numpy()) for b in h_buf]
        h_ptr = [b.data_ptr() for b in h_buf]
        done, inflated_ev = [None, None], [None, None]
        copy = torch.cuda.Stream(dev)
        copy.wait_stream(main)
        n, comp, inflated = _C.c_int64(0), _C.c_size_t(0), _C.c_int64(0)
        file_at, blocks_at, dst_at, carry, i = 0, 0, 0, b'', 0
        while file_at < size or carry:
            slot = i % 2
            if done[slot] is not None:
                done[slot].synchronize()                        # the buffer's last copy has left it
            window = views[slot][desc_bytes:]
            have = len(carry)
            window[:have] = carry
            want = min(cap - have, size - file_at)
            while want:
                got = fh.readinto(window[have:have + want])
                if not got:
                    raise IOError('%s ended %d bytes early' % (path, size - file_at))
                have, want, file_at = have + got, want - got, file_at + got
            more = file_at < size
            launches, at, nd = [], 0, 0                          # (first descriptor, blocks, inflated bytes) per launch
            while at < have and nd < desc_cap:
                _lib.check(lib.besst_bgzf_scan_chunk(p(h_ptr[slot] + desc_bytes), have, at, 1 if more else 0,
                                                     min(per_launch, desc_cap - nd), 0, p(h_ptr[slot] + nd * BGZF_DESC_BYTES),
                                                     _C.byref(n), _C.byref(comp), _C.byref(inflated)), 'besst_bgzf_scan_chunk')
                if not n.value:
                    break                                        # the window's end cuts the next block
                launches.append((nd, n.value, inflated.value))
                nd, at = nd + n.value, at + comp.value
            if not launches:
                raise IOError('%s changed while it was read' % path)
            carry = bytes(window[at:have])
            with torch.cuda.stream(copy):
                if inflated_ev[slot] is not None:
                    copy.wait_event(inflated_ev[slot])           # the launches that last read this device buffer
                d_buf[slot][:nd * BGZF_DESC_BYTES].copy_(h_buf[slot][:nd * BGZF_DESC_BYTES], non_blocking=True)
                d_buf[slot][desc_bytes:desc_bytes + at].copy_(h_buf[slot][desc_bytes:desc_bytes + at], non_blocking=True)
                done[slot] = torch.cuda.Event()
                done[slot].record(copy)
            main.wait_event(done[slot])
            d_ptr = d_buf[slot].data_ptr()
            for d0, nb, nbytes in launches:
                if blocks_at + nb > n_blocks or dst_at + nbytes > total:
                    raise IOError('%s changed while it was read' % path)
                _lib.check(lib.besst_dev_bgzf_inflate(p(main.cuda_stream), p(d_ptr + desc_bytes), p(d_ptr + d0 * BGZF_DESC_BYTES), nb,
                                                      blocks_at, nbytes, p(text.data_ptr() + dst_at), p(ws.data_ptr()), ws_bytes,
                                                      p(first_bad.data_ptr())), 'besst_dev_bgzf_inflate')
                blocks_at, dst_at = blocks_at + nb, dst_at + nbytes
            inflated_ev[slot] = torch.cuda.Event()
            inflated_ev[slot].record(main)
            i += 1
        copy.synchronize()
        main.synchronize()                                       # the pinned and the device buffers are let go here
    if blocks_at != n_blocks or dst_at != total:
        raise IOError('%s changed while it was read' % path)
    bad = _first_bad(first_bad)
    if bad is None:
        return text, total
    block, reason = bad
    if reason not in (BGZF_BAD_SIZE, BGZF_BAD_CRC):
        return None
    offset = bgzf_walk(path, block)[2]
    raise FastaError('the BGZF block at byte %d of the compressed FASTA file (block %d) is damaged: %s' % (
        offset, block, 'its CRC-32 is not that of its inflated bytes' if reason == BGZF_BAD_CRC
        else 'it does not inflate to ISIZE bytes'), offset)


GZIP_CHUNK_BYTES = 65536                 # compressed bytes per chunk of the device's gzip inflate
GZIP_INFO_WORDS = 8                      # include/besst_amd.h: BESST_GZIP_INFO_*
GZIP_MEMBER_INFO_WORDS = 16              # BESST_GZIP_MEMBER_INFO_WORDS: the words above, then ...
GZIP_INFO_MEMBERS, GZIP_INFO_BAD_MEMBER = 8, 10          # ... _MEMBERS, _MEMBER_CANDIDATES, _BAD_MEMBER, _BAD_MEMBER_OFFSET
GZIP_MEMBER_CAPACITY = None              # member candidates the device's list holds (None: gzip_member_capacity's rule)
GZIP_HEADER_ROOM = 1 << 17               # bytes of the file in which the member's header must end
GZIP_STATUS = ('ok', 'block_type', 'stored_length', 'code_lengths', 'oversubscribed_code', 'bad_code', 'bad_distance',
               'output_overrun', 'input_overrun', 'isize', 'crc', 'trailing_bytes', 'too_many_members')
GZIP_STEPS = (('probe', 'count', 'link'), ('decode', 'windows', 'translate', 'crc'))
GZIP_KERNEL_TIMES = None                 # a dict here (tools/time_fasta_ingest.py) is filled with the steps' milliseconds


def gzip_header_bytes(head):
    """The length of the gzip member header that ``head`` (the file's first bytes) begins with, i.e. where the DEFLATE
    data starts; None: not a header this package's device path takes (magic, CM = 8, reserved flag bits, a field that
    does not end inside ``head``).  RFC 1952: FEXTRA, FNAME, FCOMMENT and FHCRC are skipped."""
    if len(head) < 10 or head[:2] != GZIP_MAGIC or head[2] != 8 or head[3] & 0xe0:
        return None
    flg, at = head[3], 10
    if flg & 4:                                                  # FEXTRA
        if at + 2 > len(head):
            return None
        at += 2 + (head[at] | head[at + 1] << 8)
    for bit in (8, 16):                                          # FNAME, FCOMMENT: zero-terminated
        if flg & bit:
            end = head.find(b'\0', at) if at <= len(head) else -1
            if end < 0:
                return None
            at = end + 1
    if flg & 2:                                                  # FHCRC
        at += 2
    return at if at <= len(head) else None


def _gzip_steps(torch, names, call):
    """call(steps) for all steps at once, or - GZIP_KERNEL_TIMES - one by one between two events each"""
    times = GZIP_KERNEL_TIMES
    if times is None:
        call(0)
        return
    for k, name in enumerate(names):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call(1 << k)
        t1.record()
        t1.synchronize()
        times[name] = t0.elapsed_time(t1)


def gzip_member_capacity(comp_bytes):
    """The member candidates the device's list holds for a file of ``comp_bytes``: GZIP_MEMBER_CAPACITY where it is set,
    else a candidate per 256 bytes of the file and 4096 more (the workspace is sized from the file's geometry alone; a
    file of smaller members than that throughout is the host's: status 'too_many_members')."""
    if GZIP_MEMBER_CAPACITY is not None:
        return int(GZIP_MEMBER_CAPACITY)
    return int(comp_bytes) // 256 + 4096


def _upload_gzip_device(torch, dev, path, chunk_bytes, stats, max_text=None):
    """A file that is a series of gzip members, inflated on the device (csrc/gzip_stream.hip): the compressed file goes up
    as it is (_upload_file); besst_dev_gzip_members_plan finds the chunks and the members that can be decoded side by side
    and the text's size - the one read from the device in the middle -, besst_dev_gzip_members_inflate decodes, resolves
    the windows and checks every member's CRC-32.
    -> (text, n) as _upload_file, or None with stats['status'] saying why (and, where the device names one,
    stats['bad_member'] and stats['bad_member_offset']): the caller reads the file on the host, which also words the error
    where the file is damaged.  Every temporary is let go before that.  ``max_text``: a text of more bytes than this is not
    inflated - None with stats['status'] 'too_large', known from the plan before the text buffer is asked for (bamio's SAM
    reader then streams the file)."""
    lib = _lib.load()
    p = _C.c_void_p
    size = os.path.getsize(path)
    with open(path, 'rb') as fh:
        data_off = gzip_header_bytes(fh.read(GZIP_HEADER_ROOM))
    if data_off is None or size < data_off + 8:
        stats['status'] = 'header'
        return None
    cap = gzip_member_capacity(size)
    plan_bytes = lib.besst_dev_gzip_members_plan_workspace_bytes(size, data_off, chunk_bytes, cap)
    if not plan_bytes:
        stats['status'] = 'file_size'
        return None
    stream = p(torch.cuda.current_stream(dev).cuda_stream)

    def bad_member(words):
        if words[GZIP_INFO_BAD_MEMBER] >= 0:                     # (-1: the device names none)
            stats.update(bad_member=words[GZIP_INFO_BAD_MEMBER], bad_member_offset=words[GZIP_INFO_BAD_MEMBER + 1])
    try:
        comp, _ = _upload_file(torch, dev, path)
        plan = torch.empty(plan_bytes, dtype=torch.uint8, device=dev)
        info = torch.zeros(GZIP_MEMBER_INFO_WORDS, dtype=torch.int64, device=dev)
        _gzip_steps(torch, GZIP_STEPS[0], lambda steps: _lib.check(lib.besst_dev_gzip_members_plan(
            stream, p(comp.data_ptr()), size, data_off, chunk_bytes, cap, steps, p(plan.data_ptr()), plan_bytes,
            p(info.data_ptr())), 'besst_dev_gzip_members_plan'))
        words = info.cpu().tolist()                              # the one read in the middle: the text's size
        status, n, chunks, candidates, live = words[:5]
        members, member_candidates = words[GZIP_INFO_MEMBERS:GZIP_INFO_MEMBERS + 2]
        stats.update(chunks=chunks, candidates=candidates, live=live, text_bytes=n, status=GZIP_STATUS[status], members=members,
                     member_candidates=member_candidates)
        if status:
            bad_member(words)
            return None
        if max_text is not None and n > max_text:
            stats['status'] = 'too_large'
            return None
        ws_bytes = lib.besst_dev_gzip_members_inflate_workspace_bytes(n, live, members)
        if not ws_bytes:
            stats['status'] = 'file_size'
            return None
        text = torch.empty(n + EMIT_PAD, dtype=torch.uint8, device=dev)
        text[n:].zero_()
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _gzip_steps(torch, GZIP_STEPS[1], lambda steps: _lib.check(lib.besst_dev_gzip_members_inflate(
            stream, p(comp.data_ptr()), size, data_off, chunk_bytes, cap, steps, p(plan.data_ptr()), live, members, n,
            p(text.data_ptr()), p(ws.data_ptr()), ws_bytes, p(info.data_ptr())), 'besst_dev_gzip_members_inflate'))
        words = info.cpu().tolist()
        status = words[0]
        stats.update(status=GZIP_STATUS[status], plan_bytes=int(plan_bytes), workspace_bytes=int(ws_bytes))
        if status:
            bad_member(words)
        return (text, n) if not status else None
    except torch.cuda.OutOfMemoryError:
        stats['status'] = 'allocation'
        return None


def _gzip_members(fh, piece=1 << 20, base=0):
    """The inflated bytes of a file of gzip members, in pieces of at most ``piece`` bytes.  FastaError: the offset of the
    member that zlib does not inflate (its data, CRC-32 or length), that the file's end cuts, or that is no gzip member.
    ``base``: where in the file ``fh`` stands (the members behind a chain of BGZF blocks)."""
    pending, pos, d, member_at = b'', int(base), None, int(base)
    while True:
        if not pending:
            pending = fh.read(piece)
            if not pending:
                break
        if d is None:
            d, member_at = zlib.decompressobj(31), pos
        try:
            out = d.decompress(pending, piece)
        except zlib.error as exc:
            raise FastaError('the gzip member at byte %d of the compressed FASTA file does not inflate: %s' % (member_at, exc),
                             member_at)
        rest = d.unused_data if d.eof else d.unconsumed_tail
        pos += len(pending) - len(rest)
        pending = rest
        if d.eof:
            d = None
        if out:
            yield out
    while d is not None:                                         # (output zlib still holds when its input has run out)
        out = d.decompress(b'', piece)
        if not out:
            break
        yield out
        if d.eof:
            d = None
    if d is not None:
        raise FastaError('the compressed FASTA file ends inside the gzip member at byte %d' % member_at, member_at)


def _upload_gzip_host(torch, dev, path):
    """Any gzip file (several members, with or without BGZF's subfield), inflated by zlib on the host: the pieces are
    streamed into two pinned buffers and uploaded as they fill; no copy of the whole text exists on the host.
    -> (text, n) as _upload_file."""
    size = max(1, min(int(UPLOAD_CHUNK), max(1 << 16, 4 * os.path.getsize(path))))
    h_buf = [torch.empty(size, dtype=torch.uint8).pin_memory() for _ in range(2)]
    views = [memoryview(b.numpy()) for b in h_buf]
    done = [None, None]
    main = torch.cuda.current_stream(dev)
    copy = torch.cuda.Stream(dev)
    copy.wait_stream(main)
    parts, state = [], [0, 0]                                    # device pieces; [bytes in the buffer in use, buffers sent]

    def send():
        slot = state[1] % 2
        part = torch.empty(state[0], dtype=torch.uint8, device=dev)
        with torch.cuda.stream(copy):
            part.copy_(h_buf[slot][:state[0]], non_blocking=True)
            done[slot] = torch.cuda.Event()
            done[slot].record(copy)
        parts.append(part)
        state[0], state[1] = 0, state[1] + 1
        if done[state[1] % 2] is not None:
            done[state[1] % 2].synchronize()                     # the next buffer's last copy has left it

    try:
        with open(path, 'rb') as fh:
            for out in _gzip_members(fh):
                at = 0
                while at < len(out):
                    take = min(len(out) - at, size - state[0])
                    views[state[1] % 2][state[0]:state[0] + take] = out[at:at + take]
                    state[0], at = state[0] + take, at + take
                    if state[0] == size:
                        send()
        if state[0]:
            send()
    finally:
        copy.synchronize()
    main.wait_stream(copy)
    n = sum(int(part.shape[0]) for part in parts)
    text = torch.empty(n + EMIT_PAD, dtype=torch.uint8, device=dev)
    text[n:].zero_()
    at = 0
    while parts:
        part = parts.pop(0)
        text[at:at + part.shape[0]].copy_(part)
        at += int(part.shape[0])
        del part
    return text, n


def parse_fasta_text(text, n, tile_bytes=None):
    """The FASTA bytes ``text[:n]`` (uint8 device tensor with EMIT_PAD readable bytes behind them) -> dict(pool: padded
    uint8 tensor, pool_bytes, ctg_off, ctg_len, names, name_off: device tensors).  Raises ValueError the way
    SequenceStore.from_fasta documents."""
    import torch
    lib = _lib.load()
    dev = text.device
    tile = int(tile_bytes or 0)
    p = _C.c_void_p
    ws_bytes = lib.besst_dev_fasta_workspace_bytes(int(n), tile)
    if not ws_bytes:
        raise ValueError('tile_bytes must be a multiple of 1024 in 1024..65536')
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        info = torch.empty(FASTA_INFO_WORDS, dtype=torch.int64, device=dev)
        _lib.check(lib.besst_dev_fasta_scan(p(stream), p(text.data_ptr()), int(n), tile, p(ws.data_ptr()), ws_bytes,
                                            p(info.data_ptr())), 'besst_dev_fasta_scan')
        n_contigs, pool_bytes, names_bytes, first_error = info.cpu().numpy().view(np.uint64)[:4].tolist()
        if first_error != NO_ERROR:
            if int(text[first_error].item()) >= 128:
                raise FastaError('contig sequences must be ASCII: byte %d of the FASTA file is not' % first_error,
                                 first_error)
            raise FastaError('the header line at byte %d of the FASTA file has no name' % first_error, first_error)
        pool = torch.empty(pool_bytes + 2 * EMIT_PAD, dtype=torch.uint8, device=dev)
        pool[:EMIT_PAD].zero_()
        pool[EMIT_PAD + pool_bytes:].zero_()
        ctg_off = torch.empty(n_contigs, dtype=torch.int64, device=dev)
        ctg_len = torch.empty(n_contigs, dtype=torch.int32, device=dev)
        names = torch.empty(max(1, names_bytes), dtype=torch.uint8, device=dev)
        name_off = torch.empty(n_contigs + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.besst_dev_fasta_pack(p(stream), p(text.data_ptr()), int(n), tile, p(ws.data_ptr()), ws_bytes,
                                            p(info.data_ptr()), n_contigs, pool_bytes, names_bytes,
                                            p(pool.data_ptr() + EMIT_PAD), p(ctg_off.data_ptr()), p(ctg_len.data_ptr()),
                                            p(names.data_ptr()), p(name_off.data_ptr())), 'besst_dev_fasta_pack')
        if info.cpu().numpy().view(np.uint64)[4] != NO_ERROR:
            raise ValueError('a contig of 2^31 bases or more')
    return dict(pool=pool, pool_bytes=int(pool_bytes), ctg_off=ctg_off, ctg_len=ctg_len, names=names[:names_bytes],
                name_off=name_off)


class ScaffoldLayout(object):
    """Host side of PrintOutput: the scaffolds in output order (reversed(F), each sorted by position, :213-216), their
    junctions, and - once the overlaps are known - the piece table of the FASTA file.  Pure numpy / Python; no device.

    ``offsets`` / ``lengths``: where every sequence lies in the pool; ``index``: name -> row of those (None: the tuples
    of F in output order are the rows)."""

    def __init__(self, F, param, unique_id, offsets, lengths, index=None):
        K = param.max_contig_overlap
        if K < 0:
            raise ValueError('max_contig_overlap must not be negative')
        if K > MAX_CONTIG_OVERLAP_LIMIT:
            raise ValueError('max_contig_overlap above %d is not supported' % MAX_CONTIG_OVERLAP_LIMIT)
        self.max_overlap = int(K)
        self.scaffolds = [sorted(scaf, key=lambda t: t[2]) for scaf in reversed(F)]
        self.names = ['scaffold_' + str(k + 1) + '_uid_' + str(unique_id) for k in range(len(self.scaffolds))]
        two_sigma = 2 * param.std_dev_ins_size
        row, fwd, first, sep_n, fill, cand, pos, length = [], [], [], [], [], [], [], []
        for scaf in self.scaffolds:
            prev = None
            for t in scaf:
                row.append(len(row) if index is None else index[t[0]])
                fwd.append(bool(t[1]))
                first.append(prev is None)
                pos.append(t[2])
                length.append(t[3])
                if prev is None:
                    sep_n.append(False); fill.append(0); cand.append(False)
                else:
                    gap = t[2] - (prev[2] + prev[3])
                    cand.append(bool(gap <= two_sigma))
                    sep_n.append(bool(gap <= 1))
                    fill.append(0 if gap <= 1 else int(gap))
                prev = t
        self.row = np.asarray(row, dtype=np.int64)
        self.fwd = np.asarray(fwd, dtype=bool)
        self.first = np.asarray(first, dtype=bool)
        self.sep_n = np.asarray(sep_n, dtype=bool)
        self.fill = np.asarray(fill, dtype=np.int64)
        self.cand = np.flatnonzero(np.asarray(cand, dtype=bool))       # flat index of the RIGHT contig of every candidate
        self.unique_id = unique_id
        self._pos, self._length = pos, length                          # as given: text_columns() looks at them
        self.off = np.asarray(offsets, dtype=np.int64)[self.row] if len(row) else np.zeros(0, np.int64)
        self.len = np.asarray(lengths, dtype=np.int64)[self.row] if len(row) else np.zeros(0, np.int64)

    def text_columns(self):
        """The columns the device formats AGP and GFF from (csrc/emit_text.hip), all in output order: ``pos`` / ``len``
        int64, ``scaffold`` (int32 ordinal of every contig's scaffold), ``scaffold_start`` (int64 first contig of every
        scaffold) and ``gap`` (bool: the contig has a gap line in front of it).  None where the device cannot stand in for
        str(): a position or length that is not an integer or of magnitude 2^62 or more, a ``unique_id`` that is no int64."""
        uid = self.unique_id
        if isinstance(uid, bool) or not isinstance(uid, (int, np.integer)) or not -(1 << 63) <= int(uid) < 1 << 63:
            return None
        cols = []
        for values in (self._pos, self._length):
            a = np.asarray(values) if len(values) else np.zeros(0, dtype=np.int64)
            if a.dtype.kind not in 'iu' or a.ndim != 1:         # floats, bools, objects (Python ints past 64 bits)
                return None
            if a.dtype.kind == 'u':
                if a.size and int(a.max()) >= TEXT_LIMIT:
                    return None
            elif a.size and (int(a.max()) >= TEXT_LIMIT or int(a.min()) <= -TEXT_LIMIT):
                return None
            cols.append(a.astype(np.int64))
        pos, length = cols
        sizes = np.fromiter((len(scaf) for scaf in self.scaffolds), dtype=np.int64, count=len(self.scaffolds))
        start = np.zeros(len(sizes), dtype=np.int64)
        if len(sizes) > 1:
            np.cumsum(sizes[:-1], out=start[1:])
        scaffold = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
        gap = np.zeros(len(pos), dtype=bool)
        if len(pos) > 1:
            gap[1:] = ~self.first[1:] & (pos[1:] > pos[:-1] + length[:-1])
        return dict(pos=pos, len=length, scaffold=scaffold, scaffold_start=start, gap=gap)

    def candidates(self):
        """-> (left row, right row, forward bits) of the junctions whose overlap has to be computed."""
        c = self.cand
        forward = self.fwd[c - 1].astype(np.uint8) | (self.fwd[c].astype(np.uint8) << 1)
        return self.row[c - 1].astype(np.int32), self.row[c].astype(np.int32), forward

    def pieces(self, overlaps):
        """The piece table for the given raw overlaps (one per candidate).  Rows per contig: what precedes it (header,
        'n' or the 'N' run) and its body; one '\\n' row per scaffold."""
        nc, ns = len(self.row), len(self.scaffolds)
        drop = np.zeros(nc, dtype=np.int64)
        ov = np.asarray(overlaps, dtype=np.int64)
        merged = ov >= MIN_MERGE_OVERLAP
        drop[self.cand[merged]] = ov[merged]
        headers = [('>' + name + '\n').encode('ascii') for name in self.names]
        h_len = np.fromiter((len(h) for h in headers), dtype=np.int64, count=ns)
        h_off = np.zeros(ns, dtype=np.int64)
        if ns > 1:
            np.cumsum(h_len[:-1], out=h_off[1:])
        lit_n = int(h_len.sum())
        literals = np.frombuffer(b''.join(headers) + b'n\n', dtype=np.uint8)
        scaf_of = np.cumsum(self.first) - 1                           # scaffold ordinal of every contig
        pre = 2 * np.arange(nc, dtype=np.int64) + scaf_of
        n_rows = 2 * nc + ns
        src = np.zeros(n_rows, dtype=np.int64)
        length = np.zeros(n_rows, dtype=np.int64)
        mode = np.full(n_rows, PIECE_LITERAL, dtype=np.uint8)
        sep_n = self.sep_n | (drop > 0)
        # what precedes the contig
        src[pre] = np.where(self.first, h_off[scaf_of], lit_n)
        length[pre] = np.where(self.first, h_len[scaf_of], np.where(sep_n, 1, self.fill))
        mode[pre] = np.where(self.first | sep_n, PIECE_LITERAL, PIECE_FILL_N)
        # the contig, oriented, without the merged bases
        src[pre + 1] = self.off + np.where(self.fwd, drop, 0)
        length[pre + 1] = self.len - drop
        mode[pre + 1] = np.where(self.fwd, PIECE_COPY, PIECE_REVCOMP)
        # the line end of every scaffold: the one row no contig claimed
        is_nl = np.ones(n_rows, dtype=bool)
        is_nl[pre] = False
        is_nl[pre + 1] = False
        src[is_nl] = lit_n + 1
        length[is_nl] = 1
        out_off = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(length, out=out_off[1:])
        self.drop, self.body_rows = drop, pre + 1
        self.header_rows, self.newline_rows = pre[self.first], np.flatnonzero(is_nl)
        return dict(src_off=src, len=length, mode=mode, out_off=out_off, literals=literals,
                    total=int(out_off[-1]), merges=[(int(c), int(drop[c])) for c in np.flatnonzero(drop > 0)])

    def locate(self, emit_key, overlap_key):
        """The reference's first KeyError from the two kernels' error words -> (flat contig, pool offset of the byte)."""
        found = []
        if emit_key != NO_ERROR:
            c = int(np.searchsorted(self.body_rows, emit_key >> 32))
            found.append((c, (emit_key & 0xFFFFFFFF) + int(self.drop[c])))
        if overlap_key != NO_ERROR:
            found.append((int(self.cand[overlap_key >> 32]), overlap_key & 0xFFFFFFFF))
        if not found:
            return None
        c, pos = min(found)
        return c, int(self.off[c] + self.len[c] - 1 - pos)      # reversed: oriented position pos is that far from the end


def _out_buffer(torch, dev, n, pad=0):
    """A uint8 device tensor that takes ``n`` produced bytes: whole 16-byte groups (the kernels store those), one at least,
    and ``pad`` readable bytes behind them."""
    return torch.empty(max(16, (n + 15) // 16 * 16) + pad, dtype=torch.uint8, device=dev)


class ByteSource(object):
    """A file that is produced on the device, as write_chunks and source_bytes take it: ``total`` bytes on ``dev``;
    ``emit(begin, end, out, stream)`` enqueues bytes [begin, end) into the uint8 device tensor ``out`` (16-byte aligned)
    and waits for nothing; ``check()``, once after the last range has been consumed, synchronises and raises what went
    wrong in any of them."""

    def __init__(self, torch, dev, total, emit, check):
        self.torch, self.dev, self.total, self.emit, self.check = torch, dev, total, emit, check


class ScaffoldEmitter(object):
    """A layout on the device: overlaps computed, piece table uploaded; the byte source of the scaffold FASTA."""

    def __init__(self, F, param, store, unique_id, device=0):
        t0 = time.time()
        self.param = param
        if unique_id is None:
            unique_id = int(time.time())
        self.own_store = store is None
        if store is None:
            ordered = [t for scaf in reversed(F) for t in sorted(scaf, key=lambda t: t[2])]
            store = SequenceStore(range(len(ordered)), [t[4] for t in ordered], device=device)
            index = None
        else:
            index = store.index
        self.store = store
        self.torch, self.dev = _torch_device(store.device.index)
        torch, dev = self.torch, self.dev
        self.lib = _lib.load()
        self.layout = lay = ScaffoldLayout(F, param, unique_id, store.offsets, store.lengths, index)
        if self.own_store and getattr(param, 'outputs_on_gpu', False):
            store.set_names([t[0] for t in ordered])             # the device text takes the names from the store
        t1 = time.time()
        # overlaps of the candidate junctions
        left, right, forward = lay.candidates()
        self._err = torch.full((4,), -1, dtype=torch.int64, device=dev)   # [0] overlap, [2..3] emit
        n = len(left)
        if n:
            d_left, d_right = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
            d_fwd = torch.from_numpy(forward).to(dev)
            d_ov = torch.empty(n, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(self.lib.besst_dev_seq_overlaps(
                    _C.c_void_p(stream), _C.c_void_p(store.pool_ptr), store.pool_bytes, len(store),
                    _C.c_void_p(store._off.data_ptr()), _C.c_void_p(store._len.data_ptr()), n,
                    _C.c_void_p(d_left.data_ptr()), _C.c_void_p(d_right.data_ptr()), _C.c_void_p(d_fwd.data_ptr()),
                    lay.max_overlap, _C.c_void_p(d_ov.data_ptr()), _C.c_void_p(self._err.data_ptr())),
                    'besst_dev_seq_overlaps')
            overlaps = d_ov.cpu().numpy()
            if (overlaps < 0).any():
                raise BesstDeviceError('besst_dev_seq_overlaps: a junction names a contig outside the sequence store')
        else:
            overlaps = np.zeros(0, dtype=np.int32)
        self.overlaps = overlaps
        t2 = time.time()
        tab = self.table = lay.pieces(overlaps)
        self.total = tab['total']
        self._lit, self._lit_ptr = _padded_upload(torch, dev, tab['literals'])
        self._src = torch.from_numpy(tab['src_off']).to(dev)
        self._len = torch.from_numpy(tab['len']).to(dev)
        self._mode = torch.from_numpy(tab['mode']).to(dev)
        self._out_off = torch.from_numpy(tab['out_off']).to(dev)
        torch.cuda.synchronize(dev)
        t3 = time.time()
        self.seconds = dict(layout=t1 - t0, overlaps=t2 - t1, table=t3 - t2)

    def emit(self, begin, end, out, stream=None):
        """Enqueue bytes [begin, end) of the FASTA into the uint8 device tensor ``out`` (16-byte aligned)."""
        torch = self.torch
        if stream is None:
            stream = torch.cuda.current_stream(self.dev)
        p = _C.c_void_p
        _lib.check(self.lib.besst_dev_emit_scaffolds(
            p(stream.cuda_stream), p(self.store.pool_ptr), self.store.pool_bytes, p(self._lit_ptr),
            int(self.table['literals'].shape[0]), len(self.table['mode']), p(self._src.data_ptr()),
            p(self._len.data_ptr()), p(self._mode.data_ptr()), p(self._out_off.data_ptr()), int(begin), int(end),
            p(out.data_ptr()), p(self._err.data_ptr() + 16)), 'besst_dev_emit_scaffolds')

    def sequence_ranges(self):
        """Where every scaffold's sequence lies in the FASTA, from the piece table -> (offsets, lengths) int64, in the order
        of ``layout.names``: behind its header line, up to its '\\n'."""
        out_off, lay = self.table['out_off'], self.layout
        begin = out_off[lay.header_rows + 1]
        return begin, out_off[lay.newline_rows] - begin

    def report(self, window_bytes=None, min_gap=1):
        """The census of the scaffolds AS EMITTED (seqreport.census_source over this emitter's bytes): reversal, merged
        overlaps, the single 'n' joins and the 'N' fills are counted exactly as they are written -> SequenceCensus
        (partial) named by ``layout.names``.  Raises what ``check`` raises; the `merging` lines are not printed again."""
        from . import seqreport
        src = ByteSource(self.torch, self.dev, self.total, self.emit, lambda: self.check(quiet=True))
        seq_off, seq_len = self.sequence_ranges()
        words = seqreport.census_source(src, seq_off, seq_len, window_bytes, min_gap)
        return seqreport.SequenceCensus(self.layout.names, words, min_gap)

    def check(self, quiet=False):
        """After the last range: the `merging` lines the reference prints up to its first KeyError go to
        ``param.information_file`` (``quiet``: they do not), then that error is raised."""
        self.torch.cuda.synchronize(self.dev)
        err = self._err.cpu().numpy().view(np.uint64)
        if int(err[3]) != NO_ERROR:
            raise BesstDeviceError('besst_dev_emit_scaffolds: piece %d points outside its pool' % int(err[3]))
        hit = self.layout.locate(int(err[2]), int(err[0]))
        error = None if hit is None else KeyError(chr(self.store.byte_at(hit[1])))
        for c, n in self.table['merges']:
            if not quiet and (hit is None or c < hit[0]):
                print('merging {0} bp here'.format(n), file=self.param.information_file)
        if error is not None:
            raise error

    def close(self):
        if self.own_store:
            self.store.close()
        self._lit = self._src = self._len = self._mode = self._out_off = self._err = None


class _TextEmitter(object):
    """AGP and GFF of a layout on the device (csrc/emit_text.hip): columns uploaded, lines measured, byte ranges of either
    file on request.  ``make`` -> None where the host writer has to do the work."""

    @classmethod
    def make(cls, em):
        cols = em.layout.text_columns()
        if cols is None:
            return None
        try:
            pool = em.store.name_pool()
        except UnicodeEncodeError:
            return None
        return cls(em, cols, pool)

    def __init__(self, em, cols, pool):
        t0 = time.time()
        torch, dev, lay = em.torch, em.dev, em.layout
        self.torch, self.dev, self.lib = torch, dev, em.lib
        names, name_off, name_at = pool
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self._keep = [up(cols['pos']), up(cols['len']), up(lay.row), up(lay.fwd.astype(np.uint8)), up(cols['scaffold']),
                      up(cols['scaffold_start']), names, name_off]
        n = len(lay.row)
        ptrs = [t.data_ptr() if t.numel() else None for t in self._keep]
        self.cols = _lib.TextColumns(n, len(lay.scaffolds), int(lay.unique_id), len(name_at) - 1, int(name_at[-1]), *ptrs)
        p = _C.c_void_p
        with torch.cuda.device(dev):
            self.ws_bytes = self.lib.besst_dev_text_workspace_bytes(n)
            if not self.ws_bytes:
                raise BesstDeviceError('besst_dev_text_workspace_bytes: %d contigs are out of range' % n)
            self._ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
            self._info = torch.empty(TEXT_INFO_WORDS, dtype=torch.int64, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            stream = torch.cuda.current_stream(dev)
            ev[0].record(stream)
            _lib.check(self.lib.besst_dev_text_measure(p(stream.cuda_stream), _C.byref(self.cols), p(self._ws.data_ptr()),
                                                       self.ws_bytes, p(self._info.data_ptr())), 'besst_dev_text_measure')
            ev[1].record(stream)
            info = self._info.cpu().numpy().view(np.uint64)
        self.totals = (int(info[TEXT_AGP]), int(info[TEXT_GFF]))
        self._check(int(info[2]))
        self.measure_seconds = ev[0].elapsed_time(ev[1]) * 1e-3
        self.prep_seconds = time.time() - t0 - self.measure_seconds

    @staticmethod
    def _check(bad):
        if bad != NO_ERROR:
            raise BesstDeviceError('besst_dev_text: contig %d of the layout names a row, a name or a scaffold outside its '
                                   'table' % bad)

    def emit(self, which, begin, end, out, stream=None):
        """Enqueue bytes [begin, end) of the AGP (TEXT_AGP) or GFF (TEXT_GFF) file into ``out`` (uint8, 16-byte aligned)."""
        if stream is None:
            stream = self.torch.cuda.current_stream(self.dev)
        p = _C.c_void_p
        _lib.check(self.lib.besst_dev_text_emit(p(stream.cuda_stream), _C.byref(self.cols), p(self._ws.data_ptr()),
                                                self.ws_bytes, which, int(begin), int(end), p(out.data_ptr()),
                                                p(self._info.data_ptr())), 'besst_dev_text_emit')

    def file(self, which):
        """The AGP or GFF file as a byte source."""
        return ByteSource(self.torch, self.dev, self.totals[which],
                          lambda begin, end, out, stream: self.emit(which, begin, end, out, stream), self.check)

    def check(self):
        self.torch.cuda.synchronize(self.dev)
        self._check(int(self._info.cpu().numpy().view(np.uint64)[2]))

    def close(self):
        self._keep = self._ws = self._info = self.cols = None


def bgzf_chunk(chunk_bytes):
    """The largest multiple of the block payload within ``chunk_bytes`` (one block at least): chunks cut there leave every
    block of a file but its last full."""
    payload = int(BGZF_BLOCK_PAYLOAD)
    return max(1, int(chunk_bytes) // payload) * payload


class Deflater(object):
    """Device buffers of one BGZF compression of up to ``cap`` bytes (csrc/bgzf_deflate.hip): workspace, output, length."""

    def __init__(self, torch, dev, cap):
        self.torch, self.dev, self.lib = torch, dev, _lib.load()
        self.payload = int(BGZF_BLOCK_PAYLOAD)
        self.cap = int(cap)
        self.bound = self.lib.besst_dev_bgzf_deflate_bound(self.cap, self.payload, 1)
        self.ws_bytes = self.lib.besst_dev_bgzf_deflate_workspace_bytes(self.cap, self.payload)
        if not self.ws_bytes:
            raise ValueError('BGZF_BLOCK_PAYLOAD must lie in 1..65280')
        self._ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.out = torch.empty(self.bound + 16, dtype=torch.uint8, device=dev)
        self.length = torch.zeros(1, dtype=torch.int64, device=dev)

    def run(self, src, n, eof, stream=None):
        """Enqueue: the first ``n`` bytes of the uint8 device tensor ``src`` -> ``self.out`` / ``self.length``."""
        if n > self.cap:
            raise ValueError('more bytes than the buffers were made for')
        if stream is None:
            stream = self.torch.cuda.current_stream(self.dev)
        p = _C.c_void_p
        _lib.check(self.lib.besst_dev_bgzf_deflate(p(stream.cuda_stream), p(src.data_ptr()), int(n), self.payload, 1 if eof else 0,
                                                   p(self._ws.data_ptr()), self.ws_bytes, p(self.out.data_ptr()), self.bound,
                                                   p(self.length.data_ptr()), None), 'besst_dev_bgzf_deflate')


def bgzf_compress(data, block_payload=None, eof=True, device=0):
    """``data`` (bytes-like) as a BGZF file, compressed on the device through the library's host hook
    (besst_bgzf_deflate_device).  ``block_payload``: input bytes per block, BGZF_BLOCK_PAYLOAD by default; ``eof``: the
    28-byte EOF block is appended."""
    payload = int(BGZF_BLOCK_PAYLOAD if block_payload is None else block_payload)
    lib = _lib.load()
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    bound = lib.besst_dev_bgzf_deflate_bound(int(raw.shape[0]), payload, 1 if eof else 0)
    if not 1 <= payload <= 65280:
        raise ValueError('block_payload must lie in 1..65280')
    out = np.empty(max(1, bound), dtype=np.uint8)
    n = _C.c_size_t(0)
    _lib.check(lib.besst_bgzf_deflate_device(int(device), _lib.ptr(raw) if raw.shape[0] else None, int(raw.shape[0]), payload,
                                             1 if eof else 0, _lib.ptr(out), int(bound), _C.byref(n)), 'besst_bgzf_deflate_device')
    return out[:n.value].tobytes()


def chunk_plan(total, chunk_bytes, deflate):
    """How a file of ``total`` bytes is cut into chunks -> [(begin, end, is_last)].  Plain: at every ``chunk_bytes``.
    Deflated: at every bgzf_chunk(chunk_bytes), whole blocks, so that only the file's last block is short; an empty file is
    one empty chunk, the one that carries the EOF block."""
    step = bgzf_chunk(chunk_bytes) if deflate else max(1, int(chunk_bytes))
    if deflate and not total:
        return [(0, 0, True)]
    return [(begin, min(total, begin + step), begin + step >= total) for begin in range(0, total, step)]


def write_chunks(src, fh, chunk_bytes, deflate=False):
    """The one way of a byte source to the host: emit -> device buffer (``deflate``: -> BGZF blocks on the device,
    csrc/bgzf_deflate.hip) -> pinned buffer -> ``fh``, a binary file object, then ``src.check()``.  Two slots of every
    buffer: the kernels of chunk c + 1 are enqueued before the host waits for anything of chunk c, whose copy and file
    write run meanwhile.  Plain, the copy is enqueued right behind the kernel; deflated, the chunk's length comes back
    first and then only that many bytes.
    -> dict(emit_kernels, bgzf_kernels, d2h, file_write: seconds; file_bytes: bytes written)"""
    torch, dev = src.torch, src.dev
    plan = chunk_plan(src.total, chunk_bytes, deflate)
    spent = dict(emit_kernels=0.0, bgzf_kernels=0.0, d2h=0.0, file_write=0.0, file_bytes=0)
    with torch.cuda.device(dev):
        cap = max([1] + [end - begin for begin, end, _last in plan])
        slots = range(min(2, len(plan)))
        # (the compressor reads whole words: up to 3 bytes behind its input)
        d_buf = [_out_buffer(torch, dev, cap, EMIT_PAD if deflate else 0) for _ in slots]
        press = [Deflater(torch, dev, cap) for _ in slots] if deflate else None
        h_buf = [torch.empty(press[0].bound if deflate else cap, dtype=torch.uint8).pin_memory() for _ in slots]
        h_len = [torch.zeros(1, dtype=torch.int64).pin_memory() for _ in slots] if deflate else None
        compute, copy = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        timed = lambda: torch.cuda.Event(enable_timing=True)

        def copy_back(slot, n, source):
            with torch.cuda.stream(copy):
                c0, c1 = timed(), timed()
                c0.record(copy)
                h_buf[slot][:n].copy_(source[:n], non_blocking=True)
                c1.record(copy)
            return c0, c1

        def enqueue(slot, begin, end, last):
            k0, k1 = timed(), timed()
            k0.record(compute)
            if end > begin:
                src.emit(begin, end, d_buf[slot], compute)
            k1.record(compute)
            if not deflate:
                copy.wait_event(k1)
                return slot, end - begin, k0, k1, None, copy_back(slot, end - begin, d_buf[slot])
            press[slot].run(d_buf[slot], end - begin, last, compute)
            k2 = timed()
            k2.record(compute)
            copy.wait_event(k2)
            with torch.cuda.stream(copy):
                h_len[slot].copy_(press[slot].length, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(copy)
            return slot, None, k0, k1, k2, ready

        def drain(slot, n, k0, k1, k2, copied):
            if deflate:
                copied.synchronize()                             # the chunk's length is on the host
                n = int(h_len[slot][0])
                copied = copy_back(slot, n, press[slot].out)
                spent['bgzf_kernels'] += k1.elapsed_time(k2) * 1e-3
            copied[1].synchronize()                              # frees this slot's buffers
            spent['emit_kernels'] += k0.elapsed_time(k1) * 1e-3
            spent['d2h'] += copied[0].elapsed_time(copied[1]) * 1e-3
            t0 = time.time()
            fh.write(memoryview(h_buf[slot].numpy())[:n])
            spent['file_write'] += time.time() - t0
            spent['file_bytes'] += n

        before = None
        for i, (begin, end, last) in enumerate(plan):
            chunk = enqueue(i % 2, begin, end, last)
            if before is not None:
                drain(*before)                                   # (the other slot: this chunk's kernels run meanwhile)
            before = chunk
        if before is not None:
            drain(*before)
    src.check()
    return spent


def write_file(src, path, chunk_bytes, deflate=False):
    """write_chunks into a new file at ``path`` -> its dict."""
    with open(path, 'wb') as fh:
        return write_chunks(src, fh, chunk_bytes, deflate)


def source_bytes(src, ranges=None):
    """The file of a byte source as bytes; ``ranges`` (a list of (begin, end)) -> a list of those ranges' bytes."""
    torch, got = src.torch, []
    with torch.cuda.device(src.dev):
        for begin, end in ([(0, src.total)] if ranges is None else ranges):
            buf = _out_buffer(torch, src.dev, end - begin)
            src.emit(begin, end, buf, torch.cuda.current_stream(src.dev))
            got.append(buf[:end - begin].cpu().numpy().tobytes())
    src.check()
    return got[0] if ranges is None else got


def scaffold_bytes(F, param, store=None, unique_id=None, chunk_bytes=None, bgzf=False):
    """The FASTA text PrintOutput would write, as bytes (``chunk_bytes``: produced in ranges of that many bytes).  ``bgzf``:
    the BGZF file PrintOutput writes with ``param.outputs_bgzf`` instead (ranges of whole blocks within ``chunk_bytes``)."""
    em = ScaffoldEmitter(F, param, store, unique_id)
    try:
        out = io.BytesIO()
        write_chunks(em, out, chunk_bytes or em.total, bgzf)
        return out.getvalue()
    finally:
        em.close()


def text_bytes(F, param, store=None, unique_id=None, ranges=None):
    """(AGP, GFF) as PrintOutput writes them with ``param.outputs_on_gpu``, as bytes; with ``ranges`` (a list of (begin,
    end)) the bytes of those ranges of each file, in a list per file.  None: the layout is left to the host writer."""
    em = ScaffoldEmitter(F, param, store, unique_id)
    try:
        text = _TextEmitter.make(em)
        if text is None:
            return None
        out = tuple(source_bytes(text.file(which), ranges) for which in (TEXT_AGP, TEXT_GFF))
        text.close()
        return out
    finally:
        em.close()


def wrapped_fasta_source(store, rows):
    """The wrapped FASTA ('>' name, lines of FASTA_LINE bases) of the store's ``rows``, in that order, as a byte source;
    its ``check()`` raises if a record did not fit its table."""
    torch, dev = _torch_device(store.device.index)
    lib = _lib.load()
    names, name_off, name_at = store.name_pool()
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    if len(rows) and (int(rows.min()) < 0 or int(rows.max()) >= len(store)):
        raise ValueError('a row outside the sequence store')
    seq_len = np.asarray(store.lengths, dtype=np.int64)[rows]
    size = 2 + (name_at[1:] - name_at[:-1])[rows] + seq_len + (seq_len + FASTA_LINE - 1) // FASTA_LINE
    rec_off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(size, out=rec_off[1:])
    d_rows, d_off = torch.from_numpy(rows).to(dev), torch.from_numpy(rec_off).to(dev)
    err = torch.full((1,), -1, dtype=torch.int64, device=dev)
    p = _C.c_void_p

    def emit(begin, end, out, stream):
        _lib.check(lib.besst_dev_wrap_fasta(
            p(stream.cuda_stream), p(store.pool_ptr), store.pool_bytes, len(store), p(store._off.data_ptr()),
            p(store._len.data_ptr()), p(names.data_ptr()), int(name_at[-1]), p(name_off.data_ptr()), len(rows),
            p(d_rows.data_ptr()), p(d_off.data_ptr()), int(begin), int(end), p(out.data_ptr()), p(err.data_ptr())),
            'besst_dev_wrap_fasta')

    def check():
        bad = int(err.cpu().numpy().view(np.uint64)[0])
        if bad != NO_ERROR:
            raise BesstDeviceError('besst_dev_wrap_fasta: record %d does not fit its table' % bad)

    return ByteSource(torch, dev, int(rec_off[-1]), emit, check)


def wrapped_fasta_bytes(store, rows, ranges=None):
    """The wrapped FASTA of ``rows`` as bytes (``ranges``: a list of (begin, end) -> a list of those ranges' bytes)."""
    return source_bytes(wrapped_fasta_source(store, rows), ranges)


def write_wrapped_fasta(store, rows, path):
    """``rows`` of the store as wrapped FASTA to ``path``: no contig passes through a Python string.
    -> write_chunks' dict"""
    return write_file(wrapped_fasta_source(store, rows), path, CHUNK_BYTES)


def _write_agp_gff(layout, agp, gff):
    """reference :153-195: coordinates from positions and lengths as given; merges and the one-letter 'n' do not show."""
    print('##gff-version 3', file=gff)
    print('##agp-version 2.0\n#lw-scaffolder output', file=agp)
    for name, scaf in zip(layout.names, layout.scaffolds):
        component = 0
        prev_end = None
        for i, (contig, direction, position, length, _seq) in enumerate(scaf):
            sign = '+' if direction else '-'
            first, last = position, position + length - 1
            if i > 0 and first - (prev_end + 1) > 0:
                gap = first - (prev_end + 1)
                component += 1
                print('\t'.join(str(x) for x in (name, prev_end + 2, first, component, 'N', gap, 'scaffold', 'yes',
                                                 'paired-ends')), file=agp)
                print('\t'.join(str(x) for x in (name, 'besst_assembly', 'gap', prev_end + 2, first, '.', '.', '.', '')),
                      file=gff)
            component += 1
            print('\t'.join(str(x) for x in (name, first + 1, last + 1, component, 'W', contig, '1', last - first + 1,
                                             sign)), file=agp)
            short = '_'.join(contig.split('_', 2)[:2])
            print('\t'.join(str(x) for x in (name, 'besst_assembly', 'contig', first + 1, last + 1, '.', sign, '.',
                                             'ID=' + contig + ';Name=' + short)), file=gff)
            prev_end = last


def PrintOutput(F, Information, output_dest, param, pass_nr, store=None, unique_id=None):
    pass_dir = param.output_directory + '/pass' + str(pass_nr)
    try:
        os.mkdir(pass_dir)
    except OSError:
        pass
    print('(super)Contigs after scaffolding: ' + str(len(F)) + '\n', file=Information)
    t_start = time.time()
    bgzf = bool(getattr(param, 'outputs_bgzf', False))
    fasta = pass_dir + '/Scaffolds-pass' + str(pass_nr) + ('.fa.gz' if bgzf else '.fa')
    em = ScaffoldEmitter(F, param, store, unique_id)
    try:
        partial = fasta + '.partial'
        try:
            spent = write_file(em, partial, CHUNK_BYTES, bgzf)
        except BaseException:
            if os.path.exists(partial):
                os.remove(partial)
            raise
        os.replace(partial, fasta)
        t0 = time.time()
        text = _TextEmitter.make(em) if getattr(param, 'outputs_on_gpu', False) else None
        split = {}
        if text is not None:
            # binary files from the device buffers, through the pipeline of the FASTA
            try:
                files = [write_file(text.file(which), pass_dir + '/info-pass' + str(pass_nr) + ext, CHUNK_BYTES)
                         for which, ext in ((TEXT_GFF, '.gff'), (TEXT_AGP, '.agp'))]
                split = dict(text='device', text_prep=text.prep_seconds,
                             text_kernels=text.measure_seconds + sum(f['emit_kernels'] for f in files),
                             text_d2h=sum(f['d2h'] for f in files), text_write=sum(f['file_write'] for f in files),
                             text_bytes=sum(text.totals))
            finally:
                text.close()
        else:
            with open(pass_dir + '/info-pass' + str(pass_nr) + '.gff', 'w') as gff, \
                    open(pass_dir + '/info-pass' + str(pass_nr) + '.agp', 'w') as agp:
                _write_agp_gff(em.layout, agp, gff)
            if getattr(param, 'outputs_on_gpu', False):
                split = dict(text='host')
        if getattr(param, 'assembly_report', False):
            from . import seqreport
            t_report = time.time()
            seqreport.write_pass_report(em, Information, pass_dir, param)
            split['assembly_report'] = time.time() - t_report
        last_timings.clear()
        last_timings.update(em.seconds, emit_kernels=spent['emit_kernels'], bgzf_kernels=spent['bgzf_kernels'],
                            d2h=spent['d2h'], file_write=spent['file_write'], fasta_file_bytes=spent['file_bytes'],
                            agp_gff=time.time() - t0, total=time.time() - t_start, fasta_bytes=em.total, **split)
    finally:
        em.close()
    return ()
