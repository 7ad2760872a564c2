#!/usr/bin/env python
"""The fifteen records of tests/golden/bam/handmade_bam.json as SAM text, written by hand from the specification (SAMv1
section 1.4: QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL, then the optional fields as TAG:TYPE:VALUE).

The same names, CIGARs and optional fields as the BAM fixture beside it, as text: POS / PNEXT are the BAM's pos + 1,
RNEXT is '=' where the mate lies on the same reference, SEQ is 'AC' repeated and QUAL '?' (Phred 30) - or '*' for the
three records without a sequence.  The expected values ARE handmade_bam.json: this script writes no expectations.  It
uses neither tests/sam_writer.py nor the product, so a shared misunderstanding of the format cannot hide.

Run:  python tests/golden/sam/make_sam_fixture.py   (writes handmade.sam next to this script)
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LONG = 'a_rather_long_reference_name_to_cross_a_block_boundary'
HEADER = ['@HD\tVN:1.4\tSO:coordinate', '@SQ\tSN:ctgA\tLN:5000', '@SQ\tSN:ctgB\tLN:12345', '@SQ\tSN:%s\tLN:70000' % LONG]
TAGS = 'NM:i:3\tMD:Z:50A49\tAS:i:97\tXS:i:-5\tZB:B:S,1,2,3\tXF:f:1.5'
SEQ, QUAL = 'AC' * 50, '?' * 100

# QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL [optional]
LINES = [
    ('r01_plain', 99, 'ctgA', 101, 60, '100M', '=', 401, 400, SEQ, QUAL, ''),
    ('r02_softclip', 147, 'ctgA', 401, 60, '5S90M5S', '=', 101, -400, SEQ, QUAL, TAGS),
    ('r03_hard_and_soft', 99, 'ctgA', 701, 37, '3H10S80M10S2H', 'ctgB', 51, 0, SEQ, QUAL, ''),
    ('r04_insertion', 163, 'ctgA', 901, 60, '50M2I48M', 'ctgB', 901, 0, SEQ, QUAL, ''),
    ('r05_deletion', 83, 'ctgB', 11, 11, '50M3D50M', 'ctgA', 4001, 0, SEQ, QUAL, TAGS),
    ('r06_skip', 99, 'ctgB', 301, 10, '30M1000N70M', '=', 2001, 1800, SEQ, QUAL, ''),
    ('r07_eq_x', 147, 'ctgB', 2001, 0, '50=2X48=', '=', 301, -1800, SEQ, QUAL, ''),
    ('r08_padding', 97, 'ctgB', 2501, 60, '40M5P60M', LONG, 11, 0, SEQ, QUAL, ''),
    ('r09_unmapped_placed', 101, 'ctgB', 3001, 0, '*', '=', 3001, 0, SEQ, QUAL, ''),
    ('r10_no_sequence', 161, 'ctgB', 3501, 60, '100M', LONG, 501, 0, '*', '*', ''),
    ('r11_no_sequence_clipped', 145, 'ctgB', 3601, 60, '10S80M10S', LONG, 601, 0, '*', '*', ''),
    # the long-CIGAR convention: the placeholder CIGAR stands, the real operations sit in CG:B:I and are never read
    ('r12_cg_tag', 97, LONG, 1001, 60, '100S150N', '=', 5001, 0, SEQ, QUAL, 'CG:B:I,960,802,640'),
    ('n' * 254, 163, LONG, 5001, 60, '100M', '=', 1001, 0, SEQ, QUAL, ''),
    ('x', 99, LONG, 60001, 60, '20S30M50S', '=', 60201, 300, SEQ, QUAL, TAGS),
    ('r15_l_seq_0_no_cigar', 77, '*', 0, 0, '*', '*', 0, 0, '*', '*', ''),
]


def sam_text():
    out = list(HEADER)
    for fields in LINES:
        out.append('\t'.join(str(f) for f in fields[:11]) + ('\t' + fields[11] if fields[11] else ''))
    return '\n'.join(out) + '\n'


def main():
    path = os.path.join(HERE, 'handmade.sam')
    with open(path, 'w', newline='\n') as fh:
        fh.write(sam_text())
    print('wrote %d records, %d bytes' % (len(LINES), os.path.getsize(path)))


if __name__ == '__main__':
    main()
