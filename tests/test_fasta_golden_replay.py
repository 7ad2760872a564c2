"""tests/golden/fasta_reader.json.gz is what the REAL reference returns on the committed inputs.

Build container only (needs the reference checkout; skipped elsewhere): every case's bytes go through the reference's
own ReadInContigseqs again, the way the generator runs it, and the contigs in dictionary order, the Information text or
the exception type must equal the stored document.  This pins tests/fasta_util.py's model (tests/test_fasta_model.py
compares it with the same file) and states that `python tests/golden/make_fasta_golden.py` leaves `git diff tests/golden`
empty.
"""
import importlib.util
import os

import pytest

from tests import fasta_util as FU
from tests.refharness import loader

needs_reference = pytest.mark.skipif(not os.path.isfile(os.path.join(loader.REFERENCE_ROOT, 'runBESST')),
                                     reason='reference checkout not present')

_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def maker():
    spec = importlib.util.spec_from_file_location('make_fasta_golden', os.path.join(_HERE, 'golden', 'make_fasta_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_reference
def test_reference_reproduces_committed_fixture(maker):
    stored = FU.load_golden()
    fn = maker.load_reference()
    assert len(stored['cases']) >= 40
    for case in stored['cases']:
        assert maker.run_reference(fn, case) == case['expect'], case['name']


@needs_reference
def test_generator_inputs_are_the_committed_inputs(maker):
    stored = FU.load_golden()
    fresh = maker.all_cases()
    assert [(c['name'], c['input'], c['filter']) for c in fresh] == \
        [(c['name'], c['input'], c['filter']) for c in stored['cases']]
