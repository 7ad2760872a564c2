"""tests/golden/scaffold_output.json.gz is what the REAL reference writes on the committed inputs.

Build container only (needs the reference checkout; skipped elsewhere): every case's stored F, K and sigma go through
the reference's own GenerateOutput.PrintOutput again, with time.time pinned as in the generator, and the files, the
Information line, the `merging` lines and the KeyError must equal the stored document.  This pins
tests/output_util.py's model (tests/test_scaffold_output.py compares it with the same file) and states that
`python tests/golden/make_output_golden.py` leaves `git diff tests/golden` empty.
"""
import importlib.util
import os

import pytest

from tests import output_util as OU
from tests.refharness import loader

needs_reference = pytest.mark.skipif(not loader.available(), reason='reference checkout not present')

_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def maker():
    spec = importlib.util.spec_from_file_location('make_output_golden',
                                                  os.path.join(_HERE, 'golden', 'make_output_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_reference
def test_reference_reproduces_committed_fixture(maker):
    stored = OU.load_golden()
    GO, mods = maker.load_reference()
    assert stored['unique_id'] == maker.UNIQUE_ID
    assert stored['rev_nuc'] == maker.rev_nuc_table(GO)
    assert len(stored['cases']) >= 15
    for case in stored['cases']:
        fresh = maker.run_reference(GO, mods, case)
        assert fresh == case['expect'], case['name']


@needs_reference
def test_generator_inputs_are_the_committed_inputs(maker):
    stored = OU.load_golden()
    fresh = maker.all_cases()
    assert [c['name'] for c in fresh] == [c['name'] for c in stored['cases']]
    for f, s in zip(fresh, stored['cases']):
        assert (f['K'], f['sigma']) == (s['K'], s['sigma'])
        assert [[list(t) for t in scaf] for scaf in f['F']] == s['F'], f['name']
