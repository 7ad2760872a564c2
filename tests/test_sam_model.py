"""No GPU: the tests' own SAM decoder (tests/sam_model.py) and writer (tests/sam_writer.py) before anything is measured
against them.  The model on the hand-written fixture gives handmade_bam.json - the values pinned from the specification
for the BAM reader, reached here through a second encoding of the same records; writer -> model round-trips goldens;
every error class raises at the offending line's offset."""
import json
import os

import numpy as np
import pytest

from tests import golden_util, sam_design, sam_model, sam_writer

HERE = os.path.dirname(os.path.abspath(__file__))
SAM = os.path.join(HERE, 'golden', 'sam', 'handmade.sam')
JSON = os.path.join(HERE, 'golden', 'bam', 'handmade_bam.json')
FIELDS = ('tid', 'pos', 'mapq', 'flag', 'mtid', 'mpos', 'tlen', 'qlen', 'rlen', 'alen')


def test_handmade_sam_gives_the_handmade_json():
    with open(SAM, 'rb') as fh:
        data = fh.read()
    with open(JSON) as fh:
        doc = json.load(fh)
    got = sam_model.decode(data)
    assert got['references'] == doc['references'] and got['lengths'] == doc['lengths']
    assert len(got['tid']) == len(doc['records']) == 15
    for i, want in enumerate(doc['records']):
        for k in FIELDS:
            assert int(got[k][i]) == want[k], (want['name'], k)
    assert got['saturated'] == 0
    names = [line.split(b'\t')[0].decode() for line in data.split(b'\n') if line and not line.startswith(b'@')]
    assert [n if len(n) < 40 else n[:8] + '..%d' % len(n) for n in names] == [r['name'] for r in doc['records']]
    cigars = [line.split(b'\t')[5].decode() for line in data.split(b'\n') if line and not line.startswith(b'@')]
    assert cigars == [r['cigar'] for r in doc['records']]


def test_fixture_is_what_its_script_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_sam_fixture', os.path.join(HERE, 'golden', 'sam', 'make_sam_fixture.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(SAM, 'rb') as fh:
        assert fh.read() == mod.sam_text().encode()


@pytest.mark.parametrize('name', ['fr_infer', 'rf_contam', 'fr_edgecases'])
@pytest.mark.parametrize('form', ['plain', 'crlf_no_final_newline_optional', 'seq_star'])
def test_writer_model_round_trip(name, form):
    _, batch = golden_util.load(name)
    kw = dict(plain={}, crlf_no_final_newline_optional=dict(eol='\r\n', final_newline=False, optional='\tNM:i:0\tXS:Z:x y',
                                                          name_len=lambda i: 1 + i % 254),
              seq_star=dict(seq_star=True))[form]
    got = sam_model.decode(sam_writer.sam_bytes(batch, **kw))
    n_ref = len(batch.references)                                # (fr_edgecases names reference ids beyond its header)
    assert got['references'][:n_ref] == list(batch.references) and got['lengths'][:n_ref] == [int(x) for x in batch.lengths]
    assert got['references'] == sam_writer.padded_references(batch)[0]
    rlen = np.maximum(np.asarray(batch.rlen), 0)
    for k in ('tid', 'mtid', 'pos', 'mpos', 'tlen', 'flag', 'mapq'):
        assert np.array_equal(got[k], np.asarray(getattr(batch, k))), k
    if form == 'seq_star':
        # without a sequence the CIGAR alone speaks: [clip S] qlen M gives qlen back, rlen 0
        assert np.array_equal(got['qlen'], np.asarray(batch.qlen)) and not got['rlen'].any()
    else:
        # qlen = l_seq - clip: what the BAM of the same batch gives (a record with qlen above rlen keeps rlen)
        clip = np.maximum(rlen - np.asarray(batch.qlen, dtype=np.int64), 0)
        assert np.array_equal(got['qlen'], np.where(rlen > 0, rlen - clip, np.asarray(batch.qlen)))
        assert np.array_equal(got['rlen'], rlen)
    assert np.array_equal(got['alen'], np.asarray(batch.qlen, dtype=np.int32))


@pytest.mark.parametrize('case', sam_design.ERROR_LINES, ids=lambda c: c[0])
@pytest.mark.parametrize('eol', ['\n', '\r\n'])
def test_error_classes_raise_at_the_lines_offset(case, eol):
    _, bad, code = case
    head = sam_design.header_bytes().decode()
    good = sam_design.GOOD_LINE
    front = head.replace('\n', eol) + (good + eol) * 3
    data = (front + bad + eol + good + eol + bad + eol).encode()
    with pytest.raises(sam_model.SamModelError) as err:
        sam_model.decode(data)
    assert (err.value.code, err.value.offset, err.value.line) == (code, len(front), head.count('\n') + 4)


def test_line_ends():
    assert sam_model.lines_of(b'a\r\nb\nc') == [(0, b'a'), (3, b'b'), (5, b'c')]
    assert sam_model.lines_of(b'a\n\n') == [(0, b'a'), (2, b'')]
    assert sam_model.lines_of(b'a\rb\n') == [(0, b'a\rb')]        # a '\r' elsewhere is a byte of the line
    assert sam_model.lines_of(b'') == []
