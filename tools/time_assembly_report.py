#!/usr/bin/env python
"""Timings of the assembly report on the assembly of the size test (tests/test_gpu_scaffold_output.py: 100 k contigs,
a scaffold FASTA past 1 GiB), all in one run:

  * the two kernels of ``census_store`` over the contig pool in one call - device events after warm-up - as bytes/s on
    1 B read per base, beside a device-to-device copy of the same bytes (2 B per byte) timed alternately; the ratio says how
    far the census is from its read floor;
  * ``ScaffoldEmitter.report``: the scaffold FASTA emitted window by window and counted (wall time, synchronised);
  * ``PrintOutput`` without and with ``param.assembly_report``;
  * ``besst_host_seq_census`` over the fetched pool: the same rule byte by byte on one CPU core (``--host_bytes`` of it).

The census of the pool is checked against ``np.bincount`` per contig class before anything is timed.

    python tools/time_assembly_report.py --out profiles/assembly_report.json
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from besst_amd import GenerateOutput as GO  # noqa: E402
from besst_amd import _lib, seqreport  # noqa: E402
from tests import output_util as OU  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'assembly_report.json'))
    ap.add_argument('--contigs', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_bytes', type=int, default=64 << 20, help='bytes of the pool the host entry is timed on')
    args = ap.parse_args()
    import torch
    asm = OU.seeded_assembly(args.contigs, 3000, 20000, 17)
    pool, offsets, lengths = asm['pool'], asm['offsets'], asm['lengths'].astype(np.int64)
    doc = dict(contigs=args.contigs, pool_bytes=int(pool.shape[0]), tile_bytes=int(_lib.load().besst_dev_seq_census_tile_bytes()))
    param = OU.Param(200, asm['sigma'], None, io.StringIO())
    with OU.store_of(asm) as store:
        dev = store.device
        census = store.report()
        # the pool is A C G T only: the class counts of a few contigs by numpy, the lengths of all
        assert census.length.tolist() == lengths.tolist() and int(census.words[:, seqreport.N:seqreport.LONGEST + 1].sum()) == 0
        for row in (0, 1, args.contigs // 2, args.contigs - 1):
            got = census.words[row, seqreport.A:seqreport.T + 1].tolist()
            seq = pool[offsets[row]:offsets[row] + lengths[row]]
            assert got == [int((seq == b).sum()) for b in b'ACGT'], row
        ev = lambda: torch.cuda.Event(enable_timing=True)
        run = seqreport.CensusRun(torch, dev, store._off, store._len, store.pool_bytes)
        src, dst = store._pool, torch.empty_like(store._pool)
        census_ms, copy_ms = [], []
        for rep in range(args.reps + 2):                         # two warm-up rounds
            a, b, c = ev(), ev(), ev()
            run._acc.zero_()
            a.record()
            run.add(store.pool_ptr, 0, store.pool_bytes)
            b.record()
            dst.copy_(src)
            c.record()
            torch.cuda.synchronize(dev)
            if rep >= 2:
                census_ms.append(a.elapsed_time(b))
                copy_ms.append(b.elapsed_time(c))
        assert run.words().tolist() == census.words.tolist()
        run.close()
        del dst
        census_s, copy_s = float(np.median(census_ms)) * 1e-3, float(np.median(copy_ms)) * 1e-3
        n = store.pool_bytes
        doc['census_store_kernels'] = dict(ms=census_s * 1e3, ms_min=min(census_ms), ms_max=max(census_ms), bytes_read=n,
                                           bytes_per_s=n / census_s, d2d_copy_ms=copy_s * 1e3,
                                           d2d_copy_bytes_per_s=2 * n / copy_s, census_time_over_copy_time=census_s / copy_s,
                                           reps=args.reps)
        # the scaffolds as emitted
        em = GO.ScaffoldEmitter(asm['F'], param, store, 1)
        walls = []
        for _ in range(3):
            t0 = time.time()
            scaffolds = em.report()
            walls.append(time.time() - t0)
        doc['emitter_report'] = dict(fasta_bytes=int(em.total), scaffolds=len(scaffolds), wall_s=min(walls), wall_s_first=walls[0],
                                     bytes_per_s=em.total / min(walls), window_bytes=GO.CHUNK_BYTES)
        merged = int(em.layout.drop.sum())
        em.close()
        total = scaffolds.words.sum(axis=0)
        assert int(total[seqreport.LEN] - total[seqreport.N]) == n - merged
        # the whole call: flag off, flag on
        out_dir = tempfile.mkdtemp(prefix='besst_time_')
        runs = {}
        for pass_nr, flag in ((1, False), (2, False), (3, True), (4, True)):       # (the first call pays for the pinned buffers)
            p2 = OU.Param(200, asm['sigma'], out_dir, io.StringIO())
            p2.assembly_report = flag
            p2.contig_stats = seqreport.AssemblyStats(census)
            t0 = time.time()
            GO.PrintOutput(asm['F'], io.StringIO(), out_dir, p2, pass_nr, store=store, unique_id=1)
            runs['report' if flag else 'plain'] = dict(GO.last_timings, wall_s=time.time() - t0)
            os.remove(os.path.join(out_dir, 'pass%d' % pass_nr, 'Scaffolds-pass%d.fa' % pass_nr))
        doc['print_output'] = runs
        doc['print_output_report_extra_s'] = runs['report']['wall_s'] - runs['plain']['wall_s']
        # the host entry over the first --host_bytes of the fetched pool
        rows = int(np.searchsorted(offsets + lengths, min(args.host_bytes, n), side='right'))
        host_n = int(offsets[rows - 1] + lengths[rows - 1]) if rows else 0
        acc = np.zeros((max(rows, 1), 16), dtype=np.int64)
        off64 = np.ascontiguousarray(offsets[:rows], dtype=np.int64)
        len64 = np.ascontiguousarray(lengths[:rows], dtype=np.int64)
        host_pool = np.ascontiguousarray(pool[:max(host_n, 1)])
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        t0 = time.time()
        _lib.check(_lib.load().besst_host_seq_census(p(host_pool), 0, host_n, rows, p(off64), p(len64), 1, p(acc)),
                   'besst_host_seq_census')
        host_s = time.time() - t0
        assert acc[:rows].tolist() == census.words[:rows].tolist()
        doc['host_seq_census'] = dict(bytes=host_n, rows=rows, wall_s=host_s, bytes_per_s=host_n / host_s if host_s else None,
                                      device_over_host=(n / census_s) / (host_n / host_s) if host_s and host_n else None)
    text = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
