#!/usr/bin/env python
"""What it costs and what it saves that the device ingest writes the bit planes and the candidate side stream while it
decodes (csrc/bgzf_gpu.hip: bam_decode_kernel<true>, bam_entry_scan_kernel, bam_entries_kernel).

Two files - a dense library (config C1: the insert size spans several contigs, most mates lie elsewhere) and a paired-end
one (C2) - each written once with the native writer, then read in ONE process, BESST_INGEST_LAYOUT=0 and the default
alternating: two warm-up rounds, --rounds measured ones.  Per round: wall time of the ingest (bamio.ResidentBam, device
form), of the first build_graph, and their sum; with the feature the HBM the planes, the offsets and the entry columns
take and the entry capacity reserved against the entries made.  --package_root runs the same rounds on another checkout
(the parent commit, for the comparison in the same visit): it knows no switch, so both of its columns are the parent's.

    python tools/time_ingest_layout.py --out profiles/ingest_layout.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_round(bamio, path, wl, threads, layout):
    if layout:
        os.environ.pop('BESST_INGEST_LAYOUT', None)
    else:
        os.environ['BESST_INGEST_LAYOUT'] = '0'
    os.environ['BESST_RECORD_PATH'] = '1'                    # (the fused loop: the form that reads planes and stream)
    t0 = time.perf_counter()
    bam = bamio.ResidentBam(path, threads=threads, mode='device')
    t1 = time.perf_counter()
    ctx = bam.ctx
    ctx.set_contigs(**wl['table'])
    lib = wl['lib']
    ctx.set_library(lib['read_len'], lib['ins_size_threshold'], lib['min_mapq'], lib['orientation'], lib['detect_duplicate'],
                    lib['extend_paths'], lib['no_score'])
    t2 = time.perf_counter()
    table, aligned, ctr = ctx.build_graph()
    t3 = time.perf_counter()
    out = dict(ingest_s=t1 - t0, first_build_s=t3 - t2, sum_s=(t1 - t0) + (t3 - t2), rows=int(len(table.key)), chunks=int(bam.ingest.chunks))
    if hasattr(bam, 'layout_state'):
        st = bam.layout_state()
        n = st['n_records']
        out.update(maker_launches=st['maker_launches'], n_entries=st['n_entries'], entry_capacity=st['entry_capacity'],
                   layout_hbm_bytes=3 * ((n + 7) // 8) + 4 * ((n + 16383) // 16384 + 1) + 21 * st['entry_capacity'])
    bam.close()
    return out, (table.key.copy(), table.n.copy(), table.sum_obs.copy(), np.asarray(aligned).copy())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ingest_layout.json'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--pairs', type=int, default=None, help='read pairs per file (default: all of the config, as bench.py bam_to_graph)')
    ap.add_argument('--package_root', default=REPO, help='the checkout whose besst_amd is measured')
    ap.add_argument('--label', default='this')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from besst_amd import bamio, workload
    device = torch.device('cuda', 0)
    base = '/dev/shm' if os.path.isdir('/dev/shm') else None
    tmp = tempfile.mkdtemp(prefix='besst_layout_', dir=base)
    doc = dict(label=args.label, rounds=args.rounds, warmup_rounds=2, files={})
    try:
        for kind, config in (('dense', 'C1'), ('paired_end', 'C2')):
            wl = workload.make_device(device, config, 0, pairs=args.pairs)
            batch = wl['batch']
            path = os.path.join(tmp, kind + '.bam')
            bamio.write_bam(path, batch, level=1, realistic=True)
            threads = bamio.reader_threads()
            rounds = {'off': [], 'on': []}
            first = {}
            for r in range(args.rounds + 2):
                for mode in ('off', 'on') if r % 2 == 0 else ('on', 'off'):
                    res, tab = one_round(bamio, path, wl, threads, mode == 'on')
                    if mode in first:
                        assert all(np.array_equal(a, b) for a, b in zip(tab, first[mode]))
                    first.setdefault(mode, tab)
                    if r >= 2:
                        rounds[mode].append(res)
            assert all(np.array_equal(a, b) for a, b in zip(first['off'], first['on'])), 'the two ingests build different tables'
            summary = {}
            for mode, rs in rounds.items():
                summary[mode] = {k: dict(median=float(np.median([x[k] for x in rs])), min=float(min(x[k] for x in rs)),
                                         max=float(max(x[k] for x in rs))) for k in ('ingest_s', 'first_build_s', 'sum_s')}
                for k in ('maker_launches', 'n_entries', 'entry_capacity', 'layout_hbm_bytes', 'chunks', 'rows'):
                    if k in rs[-1]:
                        summary[mode][k] = rs[-1][k]
            doc['files'][kind] = dict(config=config, records=len(batch), bam_bytes=os.path.getsize(path), summary=summary, rounds=rounds)
            del wl, batch
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    report = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(report + '\n')
    print(report)


if __name__ == '__main__':
    main()
