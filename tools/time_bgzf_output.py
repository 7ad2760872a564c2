#!/usr/bin/env python
"""Timings of the BGZF-compressed scaffold FASTA (csrc/bgzf_deflate.hip, ``param.outputs_bgzf``) on the assembly of
tools/time_scaffold_output_text.py (100 k contigs), in one process.  Fails without a GPU.

  * PrintOutput plain and compressed, alternating, ``--reps`` rounds after two warm-up rounds: wall time of each call, and
    from GenerateOutput.last_timings the emit kernels, the deflate kernels, device-to-host copy, file write and the bytes
    written; the compressed file of the last round is decompressed and compared with the plain one;
  * the three deflate kernels of one chunk (encode, scan, pack: one call of besst_dev_bgzf_deflate) by device events, next
    to a device-to-device copy of the chunk's payload in the same run;
  * the size of the compressed file next to zlib level 1 and level 6 (and libdeflate level 1 where it is installed) on the
    same blocks of the file's first 64 MiB.

    python tools/time_bgzf_output.py --out profiles/bgzf_output.json
"""
import argparse
import gzip
import io
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from besst_amd import GenerateOutput as GO  # noqa: E402
from tests import libdeflate_util  # noqa: E402
from tests import output_util as OU  # noqa: E402


def spread(values):
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bgzf_output.json'))
    ap.add_argument('--contigs', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sample', type=int, default=64 << 20, help='bytes of the FASTA the host compressors are run on')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/time_bgzf_output.py needs a GPU')
    asm = OU.seeded_assembly(args.contigs, 3000, 20000, 17)
    out_dir = tempfile.mkdtemp(prefix='besst_bgzf_')
    doc = dict(contigs=args.contigs, reps=args.reps, block_payload=GO.BGZF_BLOCK_PAYLOAD, chunk_bytes=GO.CHUNK_BYTES)
    rounds = {False: [], True: []}
    with OU.store_of(asm) as store:
        dev = store.device
        for rep in range(args.reps + 2):                         # two warm-up rounds
            for bgzf in (False, True):
                param = OU.Param(200, asm['sigma'], out_dir, io.StringIO())
                param.outputs_bgzf = bgzf
                t0 = time.time()
                GO.PrintOutput(asm['F'], io.StringIO(), out_dir, param, 1, store=store, unique_id=1)
                wall = time.time() - t0
                if rep >= 2:
                    rounds[bgzf].append(dict(GO.last_timings, wall=wall))
        plain_path = os.path.join(out_dir, 'pass1', 'Scaffolds-pass1.fa')
        with open(plain_path, 'rb') as fh:
            plain = fh.read()
        with open(plain_path + '.gz', 'rb') as fh:
            packed = fh.read()
        assert gzip.decompress(packed) == plain, 'the compressed file does not decompress to the plain one'
        assert packed.endswith(GO.BGZF_EOF)
        keys = ('wall', 'emit_kernels', 'bgzf_kernels', 'd2h', 'file_write', 'layout', 'overlaps', 'table', 'agp_gff')
        for bgzf, name in ((False, 'plain'), (True, 'bgzf')):
            doc[name] = {k + '_s': spread([r[k] for r in rounds[bgzf]]) for k in keys}
            doc[name]['fasta_bytes'] = rounds[bgzf][0]['fasta_bytes']
            doc[name]['fasta_file_bytes'] = rounds[bgzf][0]['fasta_file_bytes']
        doc['bgzf_wall_below_plain_wall'] = bool(doc['bgzf']['wall_s']['median'] < doc['plain']['wall_s']['median'])
        doc['verified_vs_plain_file'] = True
        # the three kernels of one chunk next to a device-to-device copy of its payload
        n = min(len(plain), GO.bgzf_chunk(GO.CHUNK_BYTES))
        with torch.cuda.device(dev):
            src = torch.from_numpy(np.frombuffer(plain[:n], dtype=np.uint8).copy()).to(dev)
            pad = torch.zeros(n + GO.EMIT_PAD, dtype=torch.uint8, device=dev)
            pad[:n].copy_(src)
            dst = torch.empty_like(src)
            press = GO.Deflater(torch, dev, n)
            ev = lambda: torch.cuda.Event(enable_timing=True)
            k_ms, c_ms = [], []
            for rep in range(args.reps + 2):
                a, b, c = ev(), ev(), ev()
                a.record()
                press.run(pad, n, False)
                b.record()
                dst.copy_(src)
                c.record()
                torch.cuda.synchronize(dev)
                if rep >= 2:
                    k_ms.append(a.elapsed_time(b))
                    c_ms.append(b.elapsed_time(c))
            out_n = int(press.length.item())
        doc['deflate_kernels'] = dict(payload_bytes=n, compressed_bytes=out_n, ms=spread(k_ms), d2d_copy_ms=spread(c_ms),
                                      payload_bytes_per_s=n / (float(np.median(k_ms)) * 1e-3),
                                      d2d_copy_bytes_per_s=n / (float(np.median(c_ms)) * 1e-3))
    # sizes: the same blocks of a sample through the host compressors
    sample = plain[:min(len(plain), args.sample) // GO.BGZF_BLOCK_PAYLOAD * GO.BGZF_BLOCK_PAYLOAD or len(plain)]
    blocks = [sample[at:at + GO.BGZF_BLOCK_PAYLOAD] for at in range(0, len(sample), GO.BGZF_BLOCK_PAYLOAD)]
    ours = GO.bgzf_compress(sample, eof=False)
    assert packed.startswith(ours) or len(sample) == len(plain)
    sizes = dict(sample_bytes=len(sample), blocks=len(blocks), this_compressor=len(ours))
    for level in (1, 6):
        total = 0
        for raw in blocks:
            comp = zlib.compressobj(level, zlib.DEFLATED, -15)
            total += len(comp.compress(raw) + comp.flush()) + 26
        sizes['zlib_level_%d' % level] = total
    if libdeflate_util.available():
        sizes['libdeflate_level_1'] = sum(len(libdeflate_util.deflate(raw, 1)) + 26 for raw in blocks)
    else:
        sizes['libdeflate_level_1'] = None                      # not installed
    doc['sizes'] = sizes
    for base, _dirs, names in os.walk(out_dir, topdown=False):
        for name in names:
            os.remove(os.path.join(base, name))
        os.rmdir(base)
    text = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
