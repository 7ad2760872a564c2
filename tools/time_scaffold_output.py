#!/usr/bin/env python
"""Timings of the scaffold output stage on the assembly of the size test (tests/test_gpu_scaffold_output.py:
100 k contigs, a FASTA past 1 GiB, about half of the contigs reversed):

  * emit_kernel over the whole file in one launch - device events after warm-up - as bytes/s on 2 B per emitted base
    (one read, one write) and as a fraction of a device-to-device copy of the same byte count timed in the same run,
    the two alternating;
  * seq_overlap_kernel per 10^6 junctions at K = 200 (seeded pairs of the assembly's contigs);
  * PrintOutput's wall time and its split (layout, overlaps, table, kernels, D2H, file write);
  * the numpy model of tests/output_util.py on the same host, as the CPU comparison.

    python tools/time_scaffold_output.py --out profiles/scaffold_output.json
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
from besst_amd import _lib  # noqa: E402
from tests import output_util as OU  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'scaffold_output.json'))
    ap.add_argument('--contigs', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--junctions', type=int, default=1_000_000)
    args = ap.parse_args()
    import torch
    asm = OU.seeded_assembly(args.contigs, 3000, 20000, 17)
    t0 = time.time()
    want = OU.numpy_fasta(asm['scaffolds'], asm['pool'], asm['offsets'], asm['lengths'], asm['overlaps'], asm['sigma'], 1)
    numpy_model_s = time.time() - t0
    total = int(want.shape[0])
    doc = dict(contigs=args.contigs, fasta_bytes=total, numpy_model_s=numpy_model_s,
               numpy_model_bases_per_s=total / numpy_model_s)
    param = OU.Param(200, asm['sigma'], None, io.StringIO())
    with OU.store_of(asm) as store:
        dev = store.device
        em = GO.ScaffoldEmitter(asm['F'], param, store, 1)
        assert em.total == total
        out = torch.empty((total + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        src = torch.empty_like(out)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        emit_ms, copy_ms = [], []
        for rep in range(args.reps + 2):                         # two warm-up rounds
            a, b, c = ev(), ev(), ev()
            a.record()
            em.emit(0, total, out)
            b.record()
            src.copy_(out)
            c.record()
            torch.cuda.synchronize(dev)
            if rep >= 2:
                emit_ms.append(a.elapsed_time(b))
                copy_ms.append(b.elapsed_time(c))
        em.check()
        assert np.array_equal(out[:total].cpu().numpy(), want), 'emit_kernel output differs from the numpy model'
        emit_s, copy_s = float(np.median(emit_ms)) * 1e-3, float(np.median(copy_ms)) * 1e-3
        doc['emit_kernel'] = dict(ms=emit_s * 1e3, ms_min=min(emit_ms), ms_max=max(emit_ms), bytes_moved=2 * total,
                                  bytes_per_s=2 * total / emit_s, d2d_copy_ms=copy_s * 1e3,
                                  d2d_copy_bytes_per_s=2 * total / copy_s, fraction_of_d2d_copy=copy_s / emit_s,
                                  pieces=int(len(em.table['mode'])), reps=args.reps, verified_vs_numpy_model=True)
        em.close()
        # overlap kernel: seeded junctions between the assembly's contigs
        rng = np.random.default_rng(23)
        n = args.junctions
        d = lambda x: torch.from_numpy(x).to(dev)
        left, right = d(rng.integers(0, args.contigs, n).astype(np.int32)), d(rng.integers(0, args.contigs, n).astype(np.int32))
        fwd, ov = d(rng.integers(0, 4, n).astype(np.uint8)), torch.empty(n, dtype=torch.int32, device=dev)
        err = torch.full((1,), -1, dtype=torch.int64, device=dev)
        lib, p = _lib.load(), C.c_void_p
        times = []
        for rep in range(args.reps + 2):
            a, b = ev(), ev()
            a.record()
            _lib.check(lib.besst_dev_seq_overlaps(p(torch.cuda.current_stream(dev).cuda_stream), p(store.pool_ptr),
                                                  store.pool_bytes, len(store), p(store._off.data_ptr()),
                                                  p(store._len.data_ptr()), n, p(left.data_ptr()), p(right.data_ptr()),
                                                  p(fwd.data_ptr()), 200, p(ov.data_ptr()), p(err.data_ptr())),
                       'besst_dev_seq_overlaps')
            b.record()
            torch.cuda.synchronize(dev)
            if rep >= 2:
                times.append(a.elapsed_time(b))
        doc['seq_overlap_kernel'] = dict(junctions=n, K=200, ms=float(np.median(times)),
                                         ms_per_million_junctions=float(np.median(times)) * 1e6 / n,
                                         longest_overlap_seen=int(ov.max().item()))
        # the whole call, twice (the first pays for the pinned buffers' first touch)
        out_dir = tempfile.mkdtemp(prefix='besst_time_')
        runs = []
        for pass_nr in (1, 2):
            p2 = OU.Param(200, asm['sigma'], out_dir, io.StringIO())
            t0 = time.time()
            GO.PrintOutput(asm['F'], io.StringIO(), out_dir, p2, pass_nr, store=store, unique_id=1)
            wall = time.time() - t0
            runs.append(dict(GO.last_timings, wall_s=wall))
            os.remove(os.path.join(out_dir, 'pass%d' % pass_nr, 'Scaffolds-pass%d.fa' % pass_nr))
        doc['print_output'] = runs
    text = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
