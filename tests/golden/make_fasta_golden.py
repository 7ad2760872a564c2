"""Write tests/golden/fasta_reader.json.gz: what the REAL reference's ReadInContigseqs (runBESST:45-74) returns on small
byte strings.  Build container only (needs the reference checkout):

    python tests/golden/make_fasta_golden.py

runBESST parses its command line when it is imported, so the one function definition is taken out of the file with
``ast`` and executed in memory; nothing of it is written anywhere.  Every case goes through
``io.TextIOWrapper(io.BytesIO(data), newline=None)`` - the text mode the reference opens its file in - and records

    input     the bytes, base64
    filter    -filter_contigs (None: not given)
    contigs   [[name, sequence], ...] in the order of the returned dict          } or
    error     the exception's type name                                          }
    info      what was printed to Information up to there

tests/fasta_util.py restates the rules; tests/test_fasta_model.py compares it with this file and
tests/test_fasta_golden_replay.py re-runs the reference against it.
"""
import ast
import base64
import gzip
import io
import json
import os
import random
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

from tests.refharness import loader  # noqa: E402

OUT = os.path.join(_HERE, 'fasta_reader.json.gz')
WHITESPACE = (9, 10, 11, 12, 13, 28, 29, 30, 31, 32)


def load_reference():
    """-> the reference's ReadInContigseqs, compiled from its definition alone"""
    path = os.path.join(loader.REFERENCE_ROOT, 'runBESST')
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    found = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == 'ReadInContigseqs']
    if len(found) != 1:
        raise RuntimeError('ReadInContigseqs not found in %s' % path)
    module = ast.Module(body=found, type_ignores=[])
    ast.fix_missing_locations(module)
    scope = {}
    exec(compile(module, path, 'exec'), scope)                  # noqa: S102 - the function under test, in memory only
    return scope['ReadInContigseqs']


def wrapped(lines, width):
    return b''.join(s[i:i + width] + b'\n' for s in lines for i in range(0, max(len(s), 1), width))


def all_cases():
    rng = random.Random(20240611)

    def seq(n, alphabet=b'ACGT'):
        return bytes(rng.choice(alphabet) for _ in range(n))

    cases = []

    def add(name, data, filter_length=None):
        cases.append(dict(name=name, input=base64.b64encode(data).decode('ascii'), filter=filter_length))

    add('empty_file', b'')
    add('no_header', b'ACGT\nTTGA\n')
    add('no_header_no_newline', b'ACGT')
    add('only_newlines', b'\n\n\r\n')
    add('one_contig', b'>c1\nACGT\n')
    add('text_before_first_header', b'GGCC\nAA\n>c1\nACGT\n>c2\nTT\n')
    add('duplicate_name', b'>a\nAAAA\n>b\nCC\n>a\nGGG\n>c\nT\n')
    add('duplicate_of_first_name', b'>a\nAAAA\n>a\nCC\n')
    add('consecutive_headers', b'>a\n>b\n>c\nACGT\n>d\n>e\n')
    add('header_at_end', b'>a\nACGT\n>b')
    add('header_comments', b'>c1 length=4 cov=3.5\nACGT\n>c2\tflag\nTT\n>c3 \x1c x\nGG\n')
    add('header_leading_blank', b'>  c1 rest\nACGT\n>\tc2\nTT\n')
    add('nameless_header', b'>c1\nACGT\n>\nTT\n')
    add('nameless_header_blanks', b'>c1\nACGT\n>  \t \nTT\n')
    add('nameless_first_header', b'>')
    add('nameless_header_crlf', b'AC\r\n>\r\nTT\r\n')
    for width in (1, 60, 61):
        add('width_%d' % width, b'>w1\n' + wrapped([seq(183)], width) + b'>w2\n' + wrapped([seq(60)], width) + b'>w3\n'
            + wrapped([seq(61)], width))
    add('single_line_contigs', b'>s1\n' + seq(700) + b'\n>s2\n' + seq(1) + b'\n>s3\n' + seq(333) + b'\n')
    add('no_final_newline', b'>c1\nACGT\nTTGA\n>c2\nGGCC')
    add('no_final_newline_blank_tail', b'>c1\nACGT\nTT  \t')
    add('crlf', b'>c1 x\r\nACGT\r\nTTGA\r\n>c2\r\nGG\r\n')
    add('lone_cr', b'>c1 x\rACGT\rTTGA\r>c2\rGG\r')
    add('mixed_terminators', b'>c1\r\nAC\rGT\n\rTT\n\n\r\r\n>c2\n\rGG')
    add('blank_lines', b'\n>c1\n\nAC\n\n\nGT\n   \n\t\n>c2\n\nTT\n\n')
    for c in WHITESPACE:
        b = bytes([c])
        add('whitespace_%d' % c, b'>w' + b + b'rest\n' + b + b'AC' + b + b'GT' + b + b'\n' + b + b + b'TT' + b + b + b'\n>x\n' + b
            + b'\n' + b + b'>y\nG' + b + b'\n')
    add('gt_inside_line', b'>c1\nAC>GT\n >c2\nTT\n\t>c3 x\nG>\n>c4>c5\n>>\nA\n')
    add('gt_after_blank_is_sequence', b' >c1\nACGT\n')
    add('lower_case_and_iupac', b'>c1\nacgtnACGTN\nRYKMSWBDHVryk\nXx*-.\n>c2\nnnnn\n')
    add('interior_blanks', b'>c1\nAC GT\tAA\n  A  C  \n')
    add('long_name', b'>' + seq(300, b'abcdefgh_0123') + b' tail\nACGT\n')
    add('non_ascii_byte', b'>c1\nAC\xe9GT\n')
    add('many_small', b''.join(b'>k%d\n' % i + wrapped([seq(i)], 7) for i in range(34)))
    # -filter_contigs: the reference survives when nothing is dropped ...
    add('filter_nothing_dropped', b'>a\nACGTACGT\n>b\nACGTAC\n', 5)
    add('filter_equal_length_stays', b'>a\nACGTA\n>b\nACGTAC\n', 5)
    add('filter_zero', b'>a\nA\n>b\n\n', 0)
    add('filter_no_header', b'ACGTACGT\n', 3)
    # ... and raises RuntimeError (it deletes from the dict it iterates) when a contig is shorter: the deviation on record
    add('filter_drops_one', b'>a\nACGTACGT\n>b\nAC\n>c\nACGTAC\n', 5)
    add('filter_drops_empty', b'>a\n>b\nACGT\n', 1)
    return cases


def run_reference(fn, case):
    data = base64.b64decode(case['input'])
    info = io.StringIO()
    try:
        got = fn(io.TextIOWrapper(io.BytesIO(data), encoding='ascii', newline=None), case['filter'], info)
    except Exception as exc:                                     # noqa: BLE001 - the type is what is recorded
        return dict(error=type(exc).__name__, info=info.getvalue())
    return dict(contigs=[[k, v] for k, v in got.items()], info=info.getvalue())


def build():
    fn = load_reference()
    cases = all_cases()
    for case in cases:
        case['expect'] = run_reference(fn, case)
    return dict(source='runBESST:45-74 ReadInContigseqs', cases=cases)


def main():
    doc = build()
    with open(OUT, 'wb') as raw, gzip.GzipFile(fileobj=raw, mode='wb', mtime=0, filename='') as fh:
        fh.write(json.dumps(doc, sort_keys=True, indent=0).encode('ascii'))
    errors = sorted({c['expect'].get('error') for c in doc['cases']} - {None})
    print('%s: %d cases, %d bytes, errors: %s' % (OUT, len(doc['cases']), os.path.getsize(OUT), errors))


if __name__ == '__main__':
    main()
