#!/usr/bin/env python
"""Timings of the text of the output stage (csrc/emit_text.hip) on the assembly of tools/time_scaffold_output.py (100 k
contigs), in one process:

  * AGP / GFF: the host writer (GenerateOutput._write_agp_gff into two files: what PrintOutput does without
    ``param.outputs_on_gpu``) against the device path, split into column prep (ScaffoldLayout.text_columns, the uploads,
    the measuring launches' host side), kernels (device events over measure + both emissions, after two warm-up rounds),
    device-to-host copy and file write - the two alternating, medians over ``--reps`` rounds; the files are compared;
  * the emission kernels as bytes written per second next to a device-to-device copy of the same byte count;
  * repeats.fa for 10^4 contigs: one fetch per contig (SequenceRef -> SequenceStore.fetch -> _write_fasta) against
    wrap_fasta_kernel (GenerateOutput.write_wrapped_fasta), files compared.

    python tools/time_scaffold_output_text.py --out profiles/scaffold_output_text.json
"""
import argparse
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
from tests import output_util as OU  # noqa: E402


def median(values):
    return float(np.median(values))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'scaffold_output_text.json'))
    ap.add_argument('--contigs', type=int, default=100_000)
    ap.add_argument('--repeats', type=int, default=10_000)
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    import torch
    asm = OU.seeded_assembly(args.contigs, 3000, 20000, 17)
    out_dir = tempfile.mkdtemp(prefix='besst_text_')
    doc = dict(contigs=args.contigs, reps=args.reps)
    param = OU.Param(200, asm['sigma'], None, io.StringIO())
    with OU.store_of(asm) as store:
        dev = store.device
        em = GO.ScaffoldEmitter(asm['F'], param, store, 1)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        paths = [os.path.join(out_dir, n) for n in ('host.agp', 'host.gff', 'dev.agp', 'dev.gff')]
        host_s, dev_rounds = [], []
        for rep in range(args.reps + 2):                         # two warm-up rounds
            t0 = time.time()
            with open(paths[1], 'w') as gff, open(paths[0], 'w') as agp:
                GO._write_agp_gff(em.layout, agp, gff)
            t_host = time.time() - t0
            t0 = time.time()
            text = GO._TextEmitter.make(em)
            assert text is not None
            files = [GO.write_file(text.file(which), path, GO.CHUNK_BYTES)
                     for which, path in ((GO.TEXT_AGP, paths[2]), (GO.TEXT_GFF, paths[3]))]
            t_dev = time.time() - t0
            kernels = text.measure_seconds + sum(f['emit_kernels'] for f in files)
            d2h, write = sum(f['d2h'] for f in files), sum(f['file_write'] for f in files)
            totals = text.totals
            if rep >= 2:
                host_s.append(t_host)
                dev_rounds.append(dict(wall=t_dev, prep=text.prep_seconds, measure=text.measure_seconds, kernels=kernels,
                                       d2h=d2h, file_write=write,
                                       other=t_dev - text.prep_seconds - kernels - d2h - write))
            text.close()
        for a, b in ((paths[0], paths[2]), (paths[1], paths[3])):
            with open(a, 'rb') as fa, open(b, 'rb') as fb:
                assert fa.read() == fb.read(), 'the device text differs from the host writer'
        dev_s = {k: median([r[k] for r in dev_rounds]) for k in dev_rounds[0]}
        doc['agp_gff'] = dict(agp_bytes=totals[0], gff_bytes=totals[1], host_writer_s=median(host_s),
                              host_writer_s_min=min(host_s), host_writer_s_max=max(host_s), device_path_s=dev_s,
                              device_wall_s_min=min(r['wall'] for r in dev_rounds),
                              device_wall_s_max=max(r['wall'] for r in dev_rounds),
                              host_over_device=median(host_s) / dev_s['wall'], verified_vs_host_writer=True)
        # the emission kernels alone, whole files in one launch each, against a device-to-device copy of as many bytes
        text = GO._TextEmitter.make(em)
        total = sum(text.totals)
        bufs = [torch.empty((n + 15) // 16 * 16, dtype=torch.uint8, device=dev) for n in text.totals]
        src, dst = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
        emit_ms, copy_ms = [], []
        for rep in range(args.reps + 2):
            a, b, c = ev(), ev(), ev()
            a.record()
            for which in (GO.TEXT_AGP, GO.TEXT_GFF):
                text.emit(which, 0, text.totals[which], bufs[which])
            b.record()
            dst.copy_(src)
            c.record()
            torch.cuda.synchronize(dev)
            if rep >= 2:
                emit_ms.append(a.elapsed_time(b))
                copy_ms.append(b.elapsed_time(c))
        text.check()
        text.close()
        doc['text_emit_kernel'] = dict(bytes_written=total, ms=median(emit_ms), ms_min=min(emit_ms), ms_max=max(emit_ms),
                                       bytes_written_per_s=total / (median(emit_ms) * 1e-3), d2d_copy_ms=median(copy_ms),
                                       d2d_copy_bytes_written_per_s=total / (median(copy_ms) * 1e-3))
        em.close()
        # repeats.fa: 10^4 contigs of the same store
        rows = np.random.default_rng(5).permutation(args.contigs)[:args.repeats]
        lengths = {int(r): int(store.lengths[r]) for r in rows}
        fetch_s, batch_s, kernel_ms = [], [], []
        p_fetch, p_batch = os.path.join(out_dir, 'fetch.fa'), os.path.join(out_dir, 'batch.fa')
        for rep in range(3):
            t0 = time.time()
            with open(p_fetch, 'w') as fh:
                for r in rows.tolist():
                    GO._write_fasta(fh, store.name_of(r), GO.SequenceRef(store, r, lengths[r]))
            fetch_s.append(time.time() - t0)
            t0 = time.time()
            spent = GO.write_wrapped_fasta(store, rows, p_batch)
            batch_s.append(time.time() - t0)
            kernel_ms.append(spent['emit_kernels'] * 1e3)
        with open(p_fetch, 'rb') as fa, open(p_batch, 'rb') as fb:
            assert fa.read() == fb.read(), 'the wrapped FASTA differs from the per-contig writer'
        size = os.path.getsize(p_batch)
        doc['repeats_fasta'] = dict(contigs=args.repeats, bytes=size, per_contig_fetch_s=median(fetch_s),
                                    wrap_fasta_path_s=median(batch_s), wrap_fasta_kernel_ms=median(kernel_ms),
                                    wrap_fasta_kernel_bytes_written_per_s=size / (median(kernel_ms) * 1e-3),
                                    fetch_over_batch=median(fetch_s) / median(batch_s), verified_vs_per_contig_writer=True)
    for name in os.listdir(out_dir):
        os.remove(os.path.join(out_dir, name))
    os.rmdir(out_dir)
    text = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
