#!/usr/bin/env python
"""What the BAM report costs (csrc/report.hip: library_report_kernel) and that it leaves the layout alone.

Part 1, a C3-shaped stream drawn on the device (workload.make_device), coordinate-sorted and name-sorted, in ONE process, by
events, 2 warm-up + --rounds measured rounds each, interleaved:
    report    besst_dev_library_report over the eight columns (25 B/record read)
    copy      a device-to-device copy of the same eight columns (25 B/record read + written): the yardstick
    order     besst_dev_stream_order on the same stream (8 B/record read)
    cut_*     the report with one part left out (BESST_REPORT_CUT): where its time goes
and the ratio report / copy for both orders.

Part 2, a dense (C1) and a paired-end (C2) file of 1 M pairs as in tools/time_ingest_layout.py: device ingest, then the first
build_graph, with a report between the two and without, alternating, 2 warm-up + --rounds rounds, the build timed as that
tool times it ('as_is') and from an idle device ('synced').  The figure: the median first build with a report lies within
(max - min) of the rounds without one of the median without.

    python tools/time_bam_report.py --pairs 50000000 --out profiles/bam_report.json
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

CUTS = (('cut_mapq', 1), ('cut_qlen', 2), ('cut_isize', 4), ('cut_refs', 8), ('cut_digest', 16), ('cut_all_five', 31))


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), rounds_ms=[float(x) for x in ms])


def time_stream(torch, device, config, pairs, order, rounds, isize_bins):
    from besst_amd import _lib, report, workload
    lib = _lib.load()
    wl = workload.make_device(device, config, 0, pairs=pairs, order=order)
    cols = wl['cols']
    n_refs = int(wl['asm'].nc)
    rec = argparse.Namespace(n=int(cols['tid'].shape[0]), **cols)
    names = ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq', 'qlen')
    dst = {k: torch.empty_like(cols[k]) for k in names}
    word = torch.zeros(1, dtype=torch.int64, device=device)
    stream = torch.cuda.current_stream(device)

    def run_report():
        return report.dev_report_tensor(rec, n_refs, isize_bins)

    def run_copy():
        for k in names:
            dst[k].copy_(cols[k])

    def run_order():
        _lib.check(lib.besst_dev_stream_order(C.c_void_p(stream.cuda_stream), rec.n, C.c_void_p(rec.tid.data_ptr()),
                                              C.c_void_p(rec.pos.data_ptr()), C.c_void_p(word.data_ptr())), 'dev_stream_order')

    def cut(mask):
        def run():
            os.environ['BESST_REPORT_CUT'] = str(mask)
            try:
                return report.dev_report_tensor(rec, n_refs, isize_bins)
            finally:
                del os.environ['BESST_REPORT_CUT']
        return run
    variants = [('report', run_report), ('copy', run_copy), ('order', run_order)] + [(name, cut(mask)) for name, mask in CUTS]
    times = {name: [] for name, _ in variants}
    for r in range(rounds + 2):
        for name, fn in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if r >= 2:
                times[name].append(a.elapsed_time(b))
    whole = report.LibraryReport(run_report().cpu().numpy().view(np.uint64), n_refs, isize_bins)
    assert whole.n_records == rec.n and all(torch.equal(dst[k], cols[k]) for k in names)
    out = {name: stats(ms) for name, ms in times.items()}
    out.update(records=int(rec.n), n_refs=n_refs, bytes_read=25 * int(rec.n),
               report_over_copy=out['report']['median_ms'] / out['copy']['median_ms'],
               report_gb_per_s=25e-6 * rec.n / out['report']['median_ms'], copy_gb_per_s=50e-6 * rec.n / out['copy']['median_ms'],
               census={lab: [p, f] for lab, p, f in whole.census_rows()}, pair_classes=whole.pair_classes.tolist(),
               digest=['0x%016x' % w for w in whole.digest], distinct_qlen=int(np.count_nonzero(whole.qlen)),
               distinct_mapq=int(np.count_nonzero(whole.mapq)))
    return out


def first_build_rounds(torch, device, rounds):
    from besst_amd import bamio, workload
    os.environ['BESST_RECORD_PATH'] = '1'
    base = '/dev/shm' if os.path.isdir('/dev/shm') else None
    tmp = tempfile.mkdtemp(prefix='besst_report_', dir=base)
    out = {}
    try:
        for kind, config in (('dense', 'C1'), ('paired_end', 'C2')):
            wl = workload.make_device(device, config, 0, pairs=1000000)
            path = os.path.join(tmp, kind + '.bam')
            bamio.write_bam(path, wl['batch'], level=1, realistic=True)
            lib = wl['lib']
            # 'as_is': the wall time of the build_graph call, as tools/time_ingest_layout.py takes it - what is still in flight
            # on the context's stream behind the ingest is in it, unless a report's fetch has waited for it already;
            # 'synced': the device is idle when the call begins, so the time is the build's own
            got = {(m, s): [] for m in ('without', 'with') for s in ('as_is', 'synced')}
            tables = {}
            for r in range(rounds + 2):
                for sync in ('as_is', 'synced'):
                    for mode in ('without', 'with') if r % 2 == 0 else ('with', 'without'):
                        bam = bamio.ResidentBam(path, threads=bamio.reader_threads(), mode='device')
                        before = bam.layout_state()
                        t_rep = 0.0
                        if mode == 'with':
                            t0 = time.perf_counter()
                            bam.report()
                            t_rep = time.perf_counter() - t0
                            assert bam.layout_state() == before
                        bam.ctx.set_contigs(**wl['table'])
                        bam.ctx.set_library(lib['read_len'], lib['ins_size_threshold'], lib['min_mapq'], lib['orientation'],
                                            lib['detect_duplicate'], lib['extend_paths'], lib['no_score'])
                        if sync == 'synced':
                            torch.cuda.synchronize(device)
                        t0 = time.perf_counter()
                        table, aligned, ctr = bam.ctx.build_graph()
                        dt = time.perf_counter() - t0
                        state = bam.layout_state()
                        cur = (table.key.copy(), table.n.copy(), table.sum_obs.copy(), np.asarray(aligned).copy())
                        bam.close()
                        tables.setdefault('first', cur)
                        assert all(np.array_equal(a, b) for a, b in zip(cur, tables['first'])), 'a report changed the build'
                        assert state['maker_launches'] == 0
                        if r >= 2:
                            got[(mode, sync)].append(dict(first_build_s=dt, report_call_s=t_rep))
            out[kind] = dict(config=config, records=int(len(wl['batch'])))
            for sync in ('as_is', 'synced'):
                summary = {}
                for mode in ('without', 'with'):
                    v = [x['first_build_s'] for x in got[(mode, sync)]]
                    summary[mode] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), rounds=v)
                spread = summary['without']['max'] - summary['without']['min']
                shift = summary['with']['median'] - summary['without']['median']
                out[kind][sync] = dict(first_build_s=summary, spread_without_s=spread, median_shift_s=shift,
                                       within_spread=bool(abs(shift) <= spread), not_slower_by_more_than_spread=bool(shift <= spread),
                                       report_call_s_median=float(np.median([x['report_call_s'] for x in got[('with', sync)]])))
            del wl
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bam_report.json'))
    ap.add_argument('--config', default='C3')
    ap.add_argument('--pairs', type=int, default=None, help='read pairs of the stream (default: all of the config)')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--isize_bins', type=int, default=32768)
    args = ap.parse_args()
    import torch
    device = torch.device('cuda', 0)
    doc = dict(command='python tools/time_bam_report.py ' + ' '.join(sys.argv[1:]), config=args.config, rounds=args.rounds,
               warmup_rounds=2, isize_bins=args.isize_bins, streams={})
    for order in ('coordinate', 'name'):
        doc['streams'][order] = time_stream(torch, device, args.config, args.pairs, order, args.rounds, args.isize_bins)
        torch.cuda.empty_cache()
        print(order, json.dumps({k: v for k, v in doc['streams'][order].items() if k not in ('census',)}, sort_keys=True), flush=True)
    # (the generator draws the same pairs for both orders when the digests agree: then the two reports are equal, too)
    doc['same_records_in_both_orders'] = doc['streams']['coordinate']['digest'] == doc['streams']['name']['digest']
    doc['first_build_after_report'] = first_build_rounds(torch, device, args.rounds)
    text = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
