#!/usr/bin/env python
"""Timings of the contig FASTA reader on the assembly of the size test (tests/output_util.seeded_assembly: 100 k contigs,
1.15 GB) written as a FASTA file with 60-column lines:

  * the parse kernels (besst_dev_fasta_scan + besst_dev_fasta_pack, csrc/fasta.hip) on the file's bytes in HBM - device
    events, ten repetitions after two warm-up rounds - next to a device-to-device copy of the same bytes in the same run,
    the two alternating;
  * wall time of SequenceStore.from_fasta (file -> pinned buffers -> HBM -> kernels -> store);
  * wall time of the host path (cli.read_fasta + SequenceStore(names, sequences)) in the same process on the same file,
    in both orders, the page cache warm for both;
  * the same file compressed: as BGZF by GenerateOutput.bgzf_compress (from_fasta inflates it on the device) and by zlib
    at levels 1 and 6 as one plain gzip member each (from_fasta inflates them on the host, and with gzip_on_gpu=True on the
    device: csrc/gzip_stream.hip) - wall time of from_fasta on every file and path, alternating in the same rounds,
    --gz_reps rounds, median and range, with the bytes each form sends over PCIe; the device gzip path's kernels one by
    one (a run of their own) and its workspace; and cli.read_fasta on the BGZF file;
  * the same text as SEVERAL gzip members at level 6 - 16 concatenated members, and members of 1 MiB of text each (about
    1100) - on the host and on the device, in the same rounds.

    python tools/time_fasta_ingest.py --out profiles/fasta_ingest.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from besst_amd import GenerateOutput as GO  # noqa: E402
from besst_amd import _lib, cli  # noqa: E402
from tests import output_util as OU  # noqa: E402


def write_fasta(path, asm, width=60):
    pool = asm['pool']
    with open(path, 'wb') as fh:
        for name, off, length in zip(asm['names'], asm['offsets'].tolist(), asm['lengths'].tolist()):
            full = length // width * width
            lines = np.empty((length // width, width + 1), dtype=np.uint8)
            lines[:, :width] = pool[off:off + full].reshape(-1, width)
            lines[:, width] = 10
            fh.write(b'>' + name.encode('ascii') + b' length=%d\n' % length)
            fh.write(lines.tobytes())
            if full < length:
                fh.write(pool[off + full:off + length].tobytes() + b'\n')
    return os.path.getsize(path)


def device_path(path, **kw):
    t0 = time.time()
    store = GO.SequenceStore.from_fasta(path, **kw)
    return store, time.time() - t0


def host_path(path):
    t0 = time.time()
    seqs = cli.read_fasta(path)
    t1 = time.time()
    store = GO.SequenceStore(list(seqs), list(seqs.values()))
    return store, t1 - t0, time.time() - t1


def write_compressed(path, work):
    """-> {'bgzf': path, 'gzip': path (level 1), 'gzip6': path, 'gzip6_m16': path (16 members), 'gzip6_1m': path (a member
    per MiB of text)} of the FASTA at ``path``"""
    with open(path, 'rb') as fh:
        raw = fh.read()
    out = dict(bgzf=os.path.join(work, 'contigs.bgzf.fa.gz'), gzip=os.path.join(work, 'contigs.gzip.fa.gz'),
               gzip6=os.path.join(work, 'contigs.gzip6.fa.gz'), gzip6_m16=os.path.join(work, 'contigs.gzip6_m16.fa.gz'),
               gzip6_1m=os.path.join(work, 'contigs.gzip6_1m.fa.gz'))

    def member(piece):
        comp = zlib.compressobj(6, zlib.DEFLATED, 31)
        return comp.compress(piece) + comp.flush()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:         # (zlib lets go of the interpreter lock)
        for kind, size in (('gzip6_m16', -(-len(raw) // 16)), ('gzip6_1m', 1 << 20)):
            with open(out[kind], 'wb') as fh:
                for part in pool.map(member, (raw[at:at + size] for at in range(0, len(raw), size))):
                    fh.write(part)
    with open(out['bgzf'], 'wb') as fh:
        fh.write(GO.bgzf_compress(raw))
    for kind, level in (('gzip', 1), ('gzip6', 6)):
        comp = zlib.compressobj(level, zlib.DEFLATED, 31)
        with open(out[kind], 'wb') as fh:
            for at in range(0, len(raw), 64 << 20):
                fh.write(comp.compress(raw[at:at + (64 << 20)]))
            fh.write(comp.flush())
    return out


# what is timed: (name in the report, file, from_fasta's keywords)
RUNS = (('plain', 'plain', {}), ('bgzf', 'bgzf', {}), ('gzip', 'gzip', {}), ('gzip_device', 'gzip', {'gzip_on_gpu': True}),
        ('gzip6', 'gzip6', {}), ('gzip6_device', 'gzip6', {'gzip_on_gpu': True}),
        ('gzip6_m16', 'gzip6_m16', {}), ('gzip6_m16_device', 'gzip6_m16', {'gzip_on_gpu': True}),
        ('gzip6_1m', 'gzip6_1m', {}), ('gzip6_1m_device', 'gzip6_1m', {'gzip_on_gpu': True}))
COMPRESSED = ('bgzf', 'gzip', 'gzip6', 'gzip6_m16', 'gzip6_1m')


def compressed_runs(path, n, asm, reps, work):
    """from_fasta on the plain, the BGZF and the gzip file, alternating; cli.read_fasta on the BGZF file"""
    files = dict(write_compressed(path, work), plain=path)
    try:
        n_blocks = GO.bgzf_walk(files['bgzf'])[0]
        doc = dict(file_bytes={k: os.path.getsize(v) for k, v in files.items()}, bgzf_blocks=n_blocks,
                   # what crosses PCIe on the way in: the file (and 24 bytes of descriptor per block), or the inflated text
                   pcie_bytes=dict(plain=n, bgzf=os.path.getsize(files['bgzf']) + GO.BGZF_DESC_BYTES * n_blocks, gzip=n, gzip6=n,
                                   gzip6_m16=n, gzip6_1m=n, gzip_device=os.path.getsize(files['gzip']),
                                   gzip6_device=os.path.getsize(files['gzip6']), gzip6_m16_device=os.path.getsize(files['gzip6_m16']),
                                   gzip6_1m_device=os.path.getsize(files['gzip6_1m'])),
                   from_fasta_s={name: [] for name, _, _ in RUNS}, inflate={}, gzip_device={})
        for k in files.values():
            with open(k, 'rb') as fh:                            # page cache warm
                while fh.read(64 << 20):
                    pass
        for rep in range(reps):
            for kind, which, kw in RUNS:
                store, took = device_path(files[which], **kw)
                doc['from_fasta_s'][kind].append(took)
                doc['inflate'][kind] = store.inflate
                if kw:
                    doc['gzip_device'][kind] = dict(store.inflate_stats)
                if rep == 0:
                    assert store.names == asm['names'] and np.array_equal(store.lengths, asm['lengths'])
                    got = store._pool[GO.EMIT_PAD:GO.EMIT_PAD + store.pool_bytes].cpu().numpy()
                    assert np.array_equal(got, asm['pool']), 'the parsed pool of the %s file differs from the assembly' % kind
                    del got
                store.close()
                del store
        doc['from_fasta_s_median'] = {k: float(np.median(v)) for k, v in doc['from_fasta_s'].items()}
        doc['from_fasta_s_range'] = {k: [float(min(v)), float(max(v))] for k, v in doc['from_fasta_s'].items()}
        # the device gzip path's steps, each between two events and waited for: a run of its own, not one of the timed ones
        for kind, which, kw in RUNS:
            if kw:
                GO.GZIP_KERNEL_TIMES = {}
                try:
                    store, _ = device_path(files[which], **kw)
                    store.close()
                    del store
                    doc['gzip_device'][kind]['kernel_ms'] = dict(GO.GZIP_KERNEL_TIMES)
                finally:
                    GO.GZIP_KERNEL_TIMES = None
        t0 = time.time()
        seqs = cli.read_fasta(files['bgzf'])
        doc['read_fasta_bgzf_s'] = time.time() - t0
        assert list(seqs) == asm['names']
        del seqs
        doc['reps'] = reps
        return doc
    finally:
        for kind in COMPRESSED:
            if os.path.exists(files[kind]):
                os.remove(files[kind])


def write_report(doc, out):
    report = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write(report + '\n')
    print(report)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'fasta_ingest.json'))
    ap.add_argument('--contigs', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--gz_reps', type=int, default=3, help='rounds of from_fasta over the plain, the BGZF and the gzip files')
    ap.add_argument('--compressed_only', action='store_true', help='only the rounds over the compressed files')
    args = ap.parse_args()
    import torch
    asm = OU.seeded_assembly(args.contigs, 3000, 20000, 17)
    work = tempfile.mkdtemp(prefix='besst_fasta_')
    path = os.path.join(work, 'contigs.fa')
    n = write_fasta(path, asm)
    bases = int(asm['lengths'].sum())
    doc = dict(contigs=args.contigs, fasta_bytes=n, bases=bases, line_width=60)
    try:
        with open(path, 'rb') as fh:                             # page cache warm for everything below
            while fh.read(64 << 20):
                pass
        if args.compressed_only:
            doc['compressed'] = compressed_runs(path, n, asm, args.gz_reps, work)
            return write_report(doc, args.out)
        # wall times, both orders
        walls = []
        for order in (('device', 'host'), ('host', 'device')):
            run = dict(order=list(order))
            for which in order:
                if which == 'device':
                    store, run['from_fasta_s'] = device_path(path)
                    if not walls:
                        assert store.names == asm['names'] and np.array_equal(store.lengths, asm['lengths'])
                        assert np.array_equal(store.offsets, asm['offsets'])
                        got = store._pool[GO.EMIT_PAD:GO.EMIT_PAD + store.pool_bytes].cpu().numpy()
                        assert np.array_equal(got, asm['pool']), 'the parsed pool differs from the assembly'
                        del got
                else:
                    store, run['read_fasta_s'], run['sequence_store_s'] = host_path(path)
                    run['host_path_s'] = run['read_fasta_s'] + run['sequence_store_s']
                store.close()
                del store
            run['host_over_device'] = run['host_path_s'] / run['from_fasta_s']
            walls.append(run)
        doc['wall'] = walls
        doc['verified_vs_assembly'] = True
        doc['compressed'] = compressed_runs(path, n, asm, args.gz_reps, work)
        # the kernels alone, on the bytes in HBM
        dev = torch.device('cuda', 0)
        text, _ = GO._upload_file(torch, dev, path)
        lib, p = _lib.load(), C.c_void_p
        ws_bytes = lib.besst_dev_fasta_workspace_bytes(n, 0)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        info = torch.empty(GO.FASTA_INFO_WORDS, dtype=torch.int64, device=dev)
        pool = torch.zeros(bases + 2 * GO.EMIT_PAD, dtype=torch.uint8, device=dev)
        ctg_off = torch.empty(args.contigs, dtype=torch.int64, device=dev)
        ctg_len = torch.empty(args.contigs, dtype=torch.int32, device=dev)
        names_bytes = sum(len(x) for x in asm['names'])
        names = torch.empty(names_bytes, dtype=torch.uint8, device=dev)
        name_off = torch.empty(args.contigs + 1, dtype=torch.int64, device=dev)
        twin = torch.empty_like(text)
        stream = p(torch.cuda.current_stream(dev).cuda_stream)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        scan_ms, pack_ms, copy_ms = [], [], []
        for rep in range(args.reps + 2):                         # two warm-up rounds
            a, b, c, d = ev(), ev(), ev(), ev()
            a.record()
            _lib.check(lib.besst_dev_fasta_scan(stream, p(text.data_ptr()), n, 0, p(ws.data_ptr()), ws_bytes,
                                                p(info.data_ptr())), 'besst_dev_fasta_scan')
            b.record()
            _lib.check(lib.besst_dev_fasta_pack(stream, p(text.data_ptr()), n, 0, p(ws.data_ptr()), ws_bytes,
                                                p(info.data_ptr()), args.contigs, bases, names_bytes,
                                                p(pool.data_ptr() + GO.EMIT_PAD), p(ctg_off.data_ptr()),
                                                p(ctg_len.data_ptr()), p(names.data_ptr()), p(name_off.data_ptr())),
                       'besst_dev_fasta_pack')
            c.record()
            twin.copy_(text)
            d.record()
            torch.cuda.synchronize(dev)
            if rep >= 2:
                scan_ms.append(a.elapsed_time(b))
                pack_ms.append(b.elapsed_time(c))
                copy_ms.append(c.elapsed_time(d))
        assert info.cpu().tolist()[:3] == [args.contigs, bases, names_bytes]
        assert np.array_equal(pool[GO.EMIT_PAD:GO.EMIT_PAD + bases].cpu().numpy(), asm['pool'])
        scan_s, pack_s, copy_s = (float(np.median(x)) * 1e-3 for x in (scan_ms, pack_ms, copy_ms))
        doc['kernels'] = dict(scan_ms=scan_s * 1e3, pack_ms=pack_s * 1e3, total_ms=(scan_s + pack_s) * 1e3,
                              total_ms_min=min(a + b for a, b in zip(scan_ms, pack_ms)),
                              total_ms_max=max(a + b for a, b in zip(scan_ms, pack_ms)),
                              file_bytes_per_s=n / (scan_s + pack_s), d2d_copy_ms=copy_s * 1e3,
                              d2d_copy_file_bytes_per_s=n / copy_s, fraction_of_d2d_copy=copy_s / (scan_s + pack_s),
                              tile_bytes=16384, reps=args.reps)
    finally:
        os.remove(path)
        os.rmdir(work)
    write_report(doc, args.out)


if __name__ == '__main__':
    main()
