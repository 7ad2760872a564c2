#!/usr/bin/env python
"""Timings of the SAM text reader (bamio.ResidentSam, csrc/sam.hip) on the paired-end library of
tools/time_ingest_layout.py (config C2 cut to 1 M pairs = 2 M records) written as plain SAM with 100-base SEQ / QUAL, and as BAM with the
native writer.  One process, one GPU; two warm-up rounds, then --rounds measured ones, the forms alternating:

  * wall time of ResidentSam(path) and of ResidentBam(path, mode='device');
  * the four parse passes alone on the record text in HBM (one push of the whole text), by events
    (besst_ctx_sam_pass_times), as GB/s of text;
  * beside them in the same rounds: besst_dev_fasta_scan + besst_dev_fasta_pack on a FASTA of the same byte count, and a
    device-to-device copy of the same bytes.

    python tools/time_sam_ingest.py --out profiles/sam_ingest.json
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


def stats(values):
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sam_ingest.json'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--pairs', type=int, default=1_000_000, help='read pairs of the library (2 records each)')
    args = ap.parse_args()
    import torch
    from besst_amd import GenerateOutput as GO
    from besst_amd import _lib, bamio, device, workload
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    base = '/dev/shm' if os.path.isdir('/dev/shm') else None
    tmp = tempfile.mkdtemp(prefix='besst_sam_', dir=base)
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
        passes, fa_ms, copy_ms = [], [], []
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
            torch.cuda.synchronize()
            del parsed
            if r >= 2:
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
                            note='fasta_scan_pack is wall-clock between events around parse_fasta_text, its host wait and '
                                 'allocations included')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    report = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(report + '\n')
    print(report)


if __name__ == '__main__':
    main()
