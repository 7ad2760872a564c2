"""GPU: a SAM file in place of the BAM of the same records - sam_writer -> ResidentSam -> get_metrics + CreateGraph.PE
gives the metrics, graphs and object dicts of ResidentBam(bamio.write_bam(batch)); in an aligner's (shuffled) record order
the graphs stay the same and the information file carries the unsorted warning; through the command line the edge tables
and the report files are the same."""
import os

import numpy as np
import pytest

from besst_amd import CreateGraph, libmetrics, session
from tests import golden_util as GU
from tests import sam_writer
from tests.test_gpu_dropin import edge_rows, make_param

pytestmark = pytest.mark.gpu

PLAIN = ('u', 'v', 'nr_links', 'obs', 'obs_sq')


def run(records, doc, batch):
    """get_metrics + PE on open records -> everything the comparison reads"""
    param = make_param(doc['overrides'])
    info = param.information_file
    before = records.layout_state()
    libmetrics.get_metrics(records, param, info)
    metrics = {}
    for k in doc['metrics']:
        if k == 'empirical_distribution':
            ed = getattr(param, 'empirical_distribution', None)
            metrics[k] = None if ed is None else [ed[i] for i in range(len(ed))]
        else:
            metrics[k] = getattr(param, k, None)
    lens = dict(zip(batch.references, batch.lengths))
    C_dict = {n: 'A' * int(lens.get(n, 10)) for n in doc['fasta_names']}
    Contigs, Scaffolds, small_contigs, small_scaffolds = {}, {}, {}, {}
    G, G_prime = CreateGraph.PE(Contigs, Scaffolds, info, C_dict, param, small_contigs, small_scaffolds, records)
    after = records.layout_state()
    session.close_session(records)
    return dict(metrics=metrics, G=edge_rows(G, True), G_prime=edge_rows(G_prime, False),
                contigs=[[c.name, c.scaffold, c.coverage] for c in Contigs.values()],
                small_contigs=[[c.name, c.scaffold, c.coverage] for c in small_contigs.values()],
                scaffolds=list(Scaffolds), small_scaffolds=list(small_scaffolds), info=info.getvalue(), before=before, after=after)


@pytest.mark.parametrize('name', ['fr_infer', 'rf_contam', 'fr_edgecases'])
def test_sam_gives_what_the_bam_gives(name, tmp_path):
    from besst_amd import bamio
    doc, batch = GU.load(name)
    bam_path, sam_path = str(tmp_path / 'lib.bam'), str(tmp_path / 'lib.sam')
    bamio.write_bam(bam_path, batch, threads=3)
    with open(sam_path, 'wb') as fh:
        fh.write(sam_writer.sam_bytes(batch, name_len=lambda i: 1 + i % 40, optional=lambda i: '\tNM:i:%d' % (i % 3) if i % 2 else ''))
    bam = bamio.open_bam(bam_path)
    assert isinstance(bam, bamio.ResidentBam)
    try:
        want_cols = bam.ctx.fetch_records()
        want = run(bam, doc, batch)
    finally:
        bam.close()
    sam = bamio.open_bam(sam_path, chunk_bytes=1 << 20)
    assert isinstance(sam, bamio.ResidentSam) and len(sam) == len(batch)
    try:
        assert sam.ingest.chunks > 1 or os.path.getsize(sam_path) < (1 << 20)
        got_cols = sam.ctx.fetch_records()
        for k, v in want_cols.items():
            assert np.array_equal(got_cols[k], v), k
        got = run(sam, doc, batch)
    finally:
        sam.close()
    for k in ('metrics', 'G', 'G_prime', 'contigs', 'small_contigs', 'scaffolds', 'small_scaffolds'):
        assert got[k] == want[k], (name, k)
    # the decode wrote neither planes nor side stream: the first build made them
    assert (got['before']['bits_upto'], got['before']['tid_bits_upto'], got['before']['cs_upto']) == (0, 0, 0)
    assert got['before']['maker_launches'] == 0 and got['after']['maker_launches'] > 0
    assert want['before']['bits_upto'] == len(batch)             # (the BAM's device ingest did write them)
    if name == 'fr_infer':                                       # and the golden itself, as test_dropin_from_streamed_bam
        fin = doc['final']
        for k, v in doc['metrics'].items():
            assert got['metrics'][k] == v, k
        assert [{k: e[k] for k in PLAIN} for e in got['G']] == [{k: e[k] for k in PLAIN} for e in fin['G']]
        assert got['G_prime'] == [{k: e[k] for k in PLAIN} for e in fin['G_prime']]
        assert got['contigs'] == fin['contigs']
        assert got['scaffolds'] == fin['scaffolds'] and got['small_scaffolds'] == fin['small_scaffolds']


def test_an_aligners_record_order(tmp_path):
    """fr_infer's lines shuffled: the information file carries the unsorted warning, and the graphs are those of the BAM of
    the same records in the same order.  (They are not the sorted file's: BESST's duplicate detection compares a record
    with the one in front of it, CreateGraph.py:812-871, so which links count as duplicates follows the record order - in
    the reference as here.)"""
    from besst_amd import bamio
    from besst_amd.records import RecordBatch
    doc, batch = GU.load('fr_infer')
    order = np.random.RandomState(5).permutation(len(batch))
    shuffled = RecordBatch(batch.references, batch.lengths, **{c: np.ascontiguousarray(np.asarray(getattr(batch, c))[order])
                                                               for c in GU.COLS})
    sam_path, bam_path, sorted_path = str(tmp_path / 'shuffled.sam'), str(tmp_path / 'shuffled.bam'), str(tmp_path / 'sorted.sam')
    with open(sam_path, 'wb') as fh:
        fh.write(sam_writer.sam_bytes(batch, order=order.tolist()))
    with open(sorted_path, 'wb') as fh:
        fh.write(sam_writer.sam_bytes(batch))
    bamio.write_bam(bam_path, shuffled, threads=3)
    out = {}
    for form, path in (('sam', sam_path), ('bam', bam_path), ('sorted', sorted_path)):
        records = bamio.open_bam(path)
        try:
            cols = records.ctx.fetch_records()
            out[form] = run(records, doc, batch)
            out[form]['cols'] = cols
        finally:
            records.close()
    assert 'not sorted by coordinate' in out['sam']['info'] and 'not sorted by coordinate' in out['bam']['info']
    assert 'not sorted by coordinate' not in out['sorted']['info']
    for k, v in out['bam']['cols'].items():
        assert np.array_equal(out['sam']['cols'][k], v), k
    for k in ('metrics', 'G', 'G_prime', 'contigs', 'small_contigs', 'scaffolds', 'small_scaffolds'):
        assert out['sam'][k] == out['bam'][k], k


def test_cli_takes_sam(tmp_path):
    """test_cli_end_to_end's run with -f lib.sam: the same edges_G.tsv as with lib.bam; with --bam_report the five TSVs too"""
    from besst_amd import bamio, cli
    doc, batch = GU.load('fr_infer')
    bam, sam = str(tmp_path / 'lib.bam'), str(tmp_path / 'lib.sam')
    bamio.write_bam(bam, batch, threads=3)
    with open(sam, 'wb') as fh:
        fh.write(sam_writer.sam_bytes(batch))
    fasta = str(tmp_path / 'contigs.fa')
    lens = dict(zip(batch.references, batch.lengths))
    with open(fasta, 'w') as fh:
        for n in doc['fasta_names']:
            fh.write('>%s\n%s\n' % (n, 'A' * lens[n]))
    for lib, out in ((bam, 'from_bam'), (sam, 'from_sam')):
        assert cli.main(['-c', fasta, '-f', lib, '-orientation', 'fr', '-o', str(tmp_path / out), '--bam_report']) == 0
    for name in ('edges_G.tsv', 'edges_Gprime.tsv', 'bam_report.tsv', 'idxstats.tsv', 'mapq_hist.tsv', 'qlen_hist.tsv',
                 'insert_sizes.tsv'):
        a = open(str(tmp_path / 'from_bam' / 'BESST_output' / 'pass1' / name), 'rb').read()
        b = open(str(tmp_path / 'from_sam' / 'BESST_output' / 'pass1' / name), 'rb').read()
        assert a == b and len(a) > 0, name
    rows = [l.rstrip('\n').split('\t') for l in open(str(tmp_path / 'from_sam' / 'BESST_output' / 'pass1' / 'edges_G.tsv'))][1:]
    got = [(int(r[0]), r[1], int(r[2]), r[3], int(r[4]), int(r[5]), int(r[6])) for r in rows]
    assert got == [(e['u'][0], e['u'][1], e['v'][0], e['v'][1], e['nr_links'], e['obs'], e['obs_sq']) for e in doc['final']['G']]
