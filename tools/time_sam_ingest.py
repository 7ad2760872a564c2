#!/usr/bin/env python
"""Timings of the SAM text reader (bamio.ResidentSam, csrc/sam.hip) on the paired-end library of
tools/time_ingest_layout.py (config C2 cut to 1 M pairs = 2 M records) written as plain SAM with 100-base SEQ / QUAL, and as BAM with the
native writer.  One process, one GPU; two warm-up rounds, then --rounds measured ones, the forms alternating:

  * wall time of ResidentSam(path) and of ResidentBam(path, mode='device');
  * the four parse passes alone on the record text in HBM (one push of the whole text), by events
    (besst_ctx_sam_pass_times), as GB/s of text;
  * beside them in the same rounds: besst_dev_fasta_scan + besst_dev_fasta_pack on a FASTA of the same byte count, and a
    device-to-device copy of the same bytes.

  * the line cutter (besst_dev_sam_lines) over the record text, by events, in the rounds of the four passes;
  * with --keep-files DIR the library stays there as plain SAM, as BGZF (65 280-byte blocks, zlib level 6) and as one
    gzip member of level 6; a second run with --compare DIR --parent-tree TREE (a checkout of the parent commit, its
    library built) opens the three in alternating rounds by this tree and by the parent, a process each - the driver
    itself opens no GPU - and adds them to the document (the parent inflates a compressed file into HBM whole; this tree
    streams it).

    python tools/time_sam_ingest.py --out profiles/sam_ingest.json --keep-files DIR
    python tools/time_sam_ingest.py --out profiles/sam_ingest.json --compare DIR --parent-tree TREE
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def write_sam(path, batch):
    """the batch as SAM text: names r<i>, CIGAR [clip S] qlen M with clip = rlen - qlen, rlen bases and qualities (100 in
    this library), as the native BAM writer lays the same records out"""
    refs = list(batch.references)
    cols = [np.asarray(c).tolist() for c in (batch.tid, batch.mtid, batch.pos, batch.mpos, batch.tlen, batch.flag, batch.mapq,
                                             batch.qlen, batch.rlen if batch.rlen is not None else batch.qlen)]
    texts = {}
    with open(path, 'w', newline='\n') as fh:
        fh.write('@HD\tVN:1.4\tSO:coordinate\n')
        fh.write(''.join('@SQ\tSN:%s\tLN:%d\n' % (n, int(l)) for n, l in zip(refs, batch.lengths)))
        part = []
        for i, (tid, mtid, pos, mpos, tlen, flag, mapq, qlen, rlen) in enumerate(zip(*cols)):
            rlen = max(rlen, 0)
            if rlen not in texts:
                texts[rlen] = (('ACGT' * (rlen // 4 + 1))[:rlen], 'F' * rlen) if rlen else ('*', '*')
            seq, qual = texts[rlen]
            clip = rlen - qlen
            cigar = ('%dS' % clip if clip > 0 else '') + ('%dM' % qlen if qlen > 0 else '') or '*'
            part.append('r%d\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s\tNM:i:0\n' % (
                i, flag, refs[tid] if tid >= 0 else '*', pos + 1, mapq, cigar,
                '*' if mtid < 0 else ('=' if mtid == tid else refs[mtid]), mpos + 1, tlen, seq, qual))
            if len(part) == 65536:
                fh.write(''.join(part))
                part = []
        fh.write(''.join(part))
    return os.path.getsize(path)


def _bgzf_block(raw):
    import struct
    import zlib
    comp = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = comp.compress(raw) + comp.flush()
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data
            + struct.pack('<II', zlib.crc32(raw) & 0xffffffff, len(raw)))


def write_compressed(sam_path, bgzf_path, gzip_path):
    """the plain file again as BGZF (what bgzip writes: blocks of 65 280 bytes, level 6, the EOF block) and as `gzip -6`"""
    import zlib
    from multiprocessing.pool import ThreadPool
    with open(sam_path, 'rb') as fh:
        data = fh.read()
    pieces = [data[at:at + 65280] for at in range(0, len(data), 65280)]
    with ThreadPool(min(16, os.cpu_count() or 1)) as pool:      # (threads: zlib lets go of the interpreter lock)
        blocks = pool.map(_bgzf_block, pieces, chunksize=64)
    with open(bgzf_path, 'wb') as fh:
        fh.write(b''.join(blocks) + _bgzf_block(b''))
    comp = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(gzip_path, 'wb') as fh:
        for at in range(0, len(data), 16 << 20):
            fh.write(comp.compress(data[at:at + (16 << 20)]))
        fh.write(comp.flush())


def worker(tree):
    """opens the paths that come on stdin with the package of ``tree``; a JSON line per open"""
    sys.path.insert(0, tree)
    import torch
    torch.cuda.init()                                            # (torch's runtime first, as everywhere in this package's use)
    from besst_amd import bamio
    assert os.path.dirname(os.path.dirname(os.path.abspath(bamio.__file__))) == os.path.abspath(tree)
    for line in sys.stdin:
        path = line.strip()
        if not path:
            break
        t0 = time.perf_counter()
        rec = bamio.ResidentSam(path)
        took = time.perf_counter() - t0
        out = dict(seconds=took, chunks=int(rec.ingest.chunks), inflate=rec.inflate, records=len(rec),
                   bytes_h2d=int(rec.ingest.bytes_h2d))
        rec.close()
        print(json.dumps(out), flush=True)


def compare_trees(paths, trees, rounds):
    """{form: {tree: stats}}: every form opened by every tree in alternating rounds, a process per tree"""
    import subprocess
    procs = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', tree], stdin=subprocess.PIPE,
                                    stdout=subprocess.PIPE, text=True) for name, tree in trees.items()}
    walls = {form: {name: [] for name in trees} for form in paths}
    facts = {form: {} for form in paths}
    try:
        for r in range(rounds + 2):
            forms = list(paths) if r % 2 == 0 else list(paths)[::-1]
            names = list(trees) if r % 2 == 0 else list(trees)[::-1]
            for form in forms:
                for name in names:
                    procs[name].stdin.write(paths[form] + '\n')
                    procs[name].stdin.flush()
                    line = procs[name].stdout.readline()
                    if not line:
                        raise RuntimeError('the %s worker ended at %s' % (name, form))
                    got = json.loads(line)
                    facts[form][name] = {k: v for k, v in got.items() if k != 'seconds'}
                    if r >= 2:
                        walls[form][name].append(got['seconds'])
    finally:
        for proc in procs.values():
            proc.stdin.close()
            proc.wait(timeout=120)
    return {form: {name: dict(stats(walls[form][name]), **facts[form][name]) for name in trees} for form in paths}


def stats(values):
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sam_ingest.json'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--pairs', type=int, default=1_000_000, help='read pairs of the library (2 records each)')
    ap.add_argument('--keep-files', default=None, help='write the library here, as plain, BGZF and gzip -6 too, and leave it')
    ap.add_argument('--compare', default=None, help='the directory of an earlier --keep-files run: only the opens by both trees')
    ap.add_argument('--parent-tree', default=None, help='with --compare: a checkout of the parent commit with its library built')
    ap.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    if args.compare:
        with open(args.out) as fh:
            doc = json.load(fh)
        paths = {form: os.path.join(args.compare, name) for form, name in (('plain', 'lib.sam'), ('bgzf', 'lib.sam.bgzf'),
                                                                            ('gzip6', 'lib.sam.gz'))}
        cmp = compare_trees(paths, dict(this=REPO, parent=os.path.abspath(args.parent_tree)), args.rounds)
        b = cmp['bgzf']
        doc['compressed'] = dict(bytes={k: os.path.getsize(v) for k, v in paths.items()}, open_wall_s=cmp,
                                 bgzf_this_minus_parent_s=b['this']['median'] - b['parent']['median'],
                                 bgzf_parent_spread_s=b['parent']['max'] - b['parent']['min'],
                                 plain_over_bgzf=cmp['plain']['this']['median'] / b['this']['median'])
        report = json.dumps(doc, indent=1, sort_keys=True)
        with open(args.out, 'w') as fh:
            fh.write(report + '\n')
        print(report)
        return
    import torch
    from besst_amd import GenerateOutput as GO
    from besst_amd import _lib, bamio, device, workload
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    base = '/dev/shm' if os.path.isdir('/dev/shm') else None
    if args.keep_files:
        os.makedirs(args.keep_files, exist_ok=True)
    tmp = args.keep_files or tempfile.mkdtemp(prefix='besst_sam_', dir=base)
    try:
        wl = workload.make_device(dev, 'C2', 0, pairs=args.pairs)
        batch = wl['batch']
        sam_path, bam_path = os.path.join(tmp, 'lib.sam'), os.path.join(tmp, 'lib.bam')
        sam_bytes = write_sam(sam_path, batch)
        bamio.write_bam(bam_path, batch, level=1, realistic=True)
        doc = dict(config='C2', records=len(batch), sam_bytes=sam_bytes, bam_bytes=os.path.getsize(bam_path), rounds=args.rounds,
                   warmup_rounds=2)
        for p in (sam_path, bam_path):                           # page cache warm
            with open(p, 'rb') as fh:
                while fh.read(64 << 20):
                    pass
        # ---- the two opens, alternating
        walls, reference = dict(sam=[], bam=[]), None
        for r in range(args.rounds + 2):
            for form in ('sam', 'bam') if r % 2 == 0 else ('bam', 'sam'):
                t0 = time.perf_counter()
                rec = bamio.ResidentSam(sam_path) if form == 'sam' else bamio.ResidentBam(bam_path, mode='device')
                took = time.perf_counter() - t0
                if r == 0:
                    cols = rec.ctx.fetch_records()
                    if reference is None:
                        reference = cols
                    else:
                        assert all(np.array_equal(cols[k], reference[k]) for k in cols), 'SAM and BAM give different columns'
                    doc.setdefault('chunks', {})[form] = int(rec.ingest.chunks)
                rec.close()
                if r >= 2:
                    walls[form].append(took)
        doc['open_wall_s'] = {k: stats(v) for k, v in walls.items()}
        if args.keep_files:
            write_compressed(sam_path, sam_path + '.bgzf', sam_path + '.gz')
        # ---- the parse passes alone, a FASTA parse and a copy of the same bytes beside them
        with open(sam_path, 'rb') as fh:
            header, h_bytes = bamio._read_plain_header(fh)
            body = np.frombuffer(fh.read(), dtype=np.uint8)
        n = int(body.shape[0])
        text = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        text[:n].copy_(torch.from_numpy(body.copy()))
        line = np.frombuffer(b'ACGT' * 15 + b'\n', dtype=np.uint8)
        fasta = np.tile(line, n // 61 + 1)[:n].copy()
        fasta[:9] = np.frombuffer(b'>contig1\n', dtype=np.uint8)
        fa_text = torch.zeros(n + GO.EMIT_PAD, dtype=torch.uint8, device=dev)
        fa_text[:n].copy_(torch.from_numpy(fasta))
        copy_dst = torch.empty(n, dtype=torch.uint8, device=dev)
        names, _ = bamio.parse_sam_header(header)
        ctx = device.GraphContext(0)
        blobs = [x.encode() for x in names]
        off = np.zeros(len(blobs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in blobs], out=off[1:])
        pool = np.frombuffer(b''.join(blobs), dtype=np.uint8)
        _lib.check(lib.besst_ctx_set_sam_references(ctx._ctx, _lib.ptr(pool), _lib.ptr(off), len(blobs)), 'refs')
        head = [np.zeros(1000, dtype=np.int32), np.zeros(1000, dtype=np.int32), np.zeros(1000, dtype=np.uint16)]
        info = np.zeros(4, dtype=np.int64)
        passes, fa_ms, copy_ms, cut_ms = [], [], [], []
        cut_out = torch.zeros(4, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for r in range(args.rounds + 2):
            ctx.clear_records()
            _lib.check(lib.besst_ctx_sam_pass_times(ctx._ctx, 1, None), 'pass_times')
            _lib.check(lib.besst_ctx_push_sam_text(ctx._ctx, C.c_void_p(stream), C.c_void_p(text.data_ptr()), n, h_bytes, 0, 1000,
                                                   _lib.ptr(head[0]), _lib.ptr(head[1]), _lib.ptr(head[2]), _lib.ptr(info)), 'push')
            assert info[2] < 0 and info[0] == len(batch)
            ms = np.zeros(4, dtype=np.float64)
            _lib.check(lib.besst_ctx_sam_pass_times(ctx._ctx, 0, _lib.ptr(ms)), 'pass_times')
            a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            parsed = GO.parse_fasta_text(fa_text, n, None)
            b.record()
            copy_dst.copy_(text[:n])
            c.record()
            d = torch.cuda.Event(enable_timing=True)
            _lib.check(lib.besst_dev_sam_lines(C.c_void_p(stream), C.c_void_p(text.data_ptr()), n, 1, n // 2,
                                               C.c_void_p(cut_out.data_ptr())), 'sam_lines')
            d.record()
            torch.cuda.synchronize()
            assert cut_out.tolist()[:2] == [n, 0]
            del parsed
            if r >= 2:
                cut_ms.append(c.elapsed_time(d))
                passes.append(ms.tolist())
                fa_ms.append(a.elapsed_time(b))
                copy_ms.append(b.elapsed_time(c))
        ctx.close()
        passes = np.asarray(passes)
        gbs = lambda ms: n / (np.asarray(ms) * 1e-3) / 1e9
        doc['parse'] = dict(text_bytes=n,
                            pass_ms={k: stats(passes[:, i]) for i, k in enumerate(('flags', 'state', 'index', 'decode'))},
                            all_passes_ms=stats(passes.sum(axis=1)), all_passes_gb_per_s=stats(gbs(passes.sum(axis=1))),
                            fasta_scan_pack_ms=stats(fa_ms), fasta_scan_pack_gb_per_s=stats(gbs(fa_ms)),
                            device_copy_ms=stats(copy_ms), device_copy_gb_per_s=stats(gbs(copy_ms)),
                            line_cutter_ms=stats(cut_ms), line_cutter_gb_per_s=stats(gbs(cut_ms)),
                            note='fasta_scan_pack is wall-clock between events around parse_fasta_text, its host wait and '
                                 'allocations included; line_cutter is besst_dev_sam_lines with its two memsets, the '
                                 'end of the header asked for and the newlines of the first half counted')
    finally:
        if not args.keep_files:
            shutil.rmtree(tmp, ignore_errors=True)
    report = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(report + '\n')
    print(report)


if __name__ == '__main__':
    main()
