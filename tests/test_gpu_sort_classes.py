"""Stage 2 (csrc/sortreduce.hip, onesweep.hip, runs.hip) at the borders of its size classes: streams designed so that a
bucket sits on each side of every border the kernels dispatch on (tests/sort_design.py; tests/test_sort_design.py checks
the designs without a GPU).  Every test holds the edge table against oracle.c_oracle.edge_rows (numpy stable sort, exact
integer sums) - exact equality of every column, row_mask and row_offset included - AND holds besst_dev_reduce_census,
what the call really did, against the prediction: a change of a dispatch constant then fails here instead of moving the
stream to other kernels unnoticed.  Each call is made twice on one builder (run_reduce)."""
import pytest

from tests import sort_design as SD
from tests.test_gpu_runs import assert_rows, run_reduce

pytestmark = pytest.mark.gpu

NO_RUNS = 1                                                  # pipeline.REDUCE_NO_RUNS (asserted below)
ZERO_CENSUS = [0] * 7


def reduce_and_check(keys, payload, key_bits, key_base, cap, flags, want_census):
    from besst_amd import pipeline
    assert pipeline.REDUCE_NO_RUNS == NO_RUNS
    node_bits = max(1, min(29, (key_bits - 1) // 2))
    gb, n_rows = run_reduce(keys, payload, node_bits, cap=cap, flags=flags, key_bits=key_bits, key_base=key_base)
    assert gb.sort_flags == flags, 'read_sizes() repeated the call in another form'
    got = gb.reduce_census(cap or len(keys))
    assert got == list(want_census), SD.explain_census(got, want_census)
    assert_rows(gb, n_rows, keys, payload)


@pytest.mark.parametrize('key_bits,big', [(25, False), (30, False), (37, False), (41, False), (37, True)])
def test_chained_scan_buckets(key_bits, big):
    """Chained scan + buckets (BESST_REDUCE_NO_RUNS, 4.3 M slots).  9, 14, 21 and 25 key bits are left to the buckets: 2
    digit passes with a 2-bit top digit, 2 full ones, 3 (odd: the LDS sort's result lies in the scratch) and 4 with a
    partial digit.  One stream per width holds the wave kernel's template borders with 1 / 2 / 8 / 48 keys, the 48 / 49
    keys and eight-smallest-cover-a-sixth borders, the digit-pass kernel's carried rows, the workgroup kernel's 1537 ..
    20 000 words and the row mover's borders.  (With 9 low bits a bucket has 512 keys to choose from: the cases that ask for
    1535, 1536 or 4097 distinct keys hold every low key, several tuples each - labelled so; the other widths hold the real
    thing.)  With large observations (one width): squares up to 2^52, a row of 5000
    tuples summing beyond 2^32."""
    key_base = (3 << 45) + 12_345 if key_bits in (30, 41) else 0
    _, keys, payload = SD.chained_stream(key_bits, key_base=key_base, big=big)
    want = SD.chained_census(SD.predict_chained(keys, key_bits, key_base))
    reduce_and_check(keys, payload, key_bits, key_base, SD.LARGE_CAPACITY, NO_RUNS, want)


@pytest.mark.parametrize('n', [0, 1, 100])
def test_chained_scan_buckets_on_nearly_empty_streams(n):
    """The same form with 0, 1 and 100 tuples in 4.3 M slots: every bucket but a handful empty, n_rows from the row mover's
    last workgroup."""
    key_bits = 37
    keys, payload = SD.tiny_stream(n, key_bits)
    want = SD.chained_census(SD.predict_chained(keys, key_bits))
    assert want[1] >= (1 << 16) - n
    reduce_and_check(keys, payload, key_bits, 0, SD.LARGE_CAPACITY, NO_RUNS, want)


@pytest.mark.parametrize('key_bits,one_more,big', [(20, False, False), (20, True, False), (45, False, False), (45, True, False),
                                                   (20, True, True)])
def test_chained_scan_tile_reduction(key_bits, one_more, big):
    """Chained scan + os_reduce_kernel / os_fixup_kernel (BESST_REDUCE_NO_RUNS; 20-bit keys: packed, three passes; 45-bit
    keys: index arrays).  Row heads on tile offsets 0, 1 and 4095, rows of exactly one tile, two tiles and two tiles + 1,
    one row from the middle of tile 0 to the middle of tile 5 with head-less tiles between, the stream ending on a tile
    border / one tuple into a tile."""
    keys, payload = SD.tile_stream(key_bits, one_more=one_more, big=big)
    reduce_and_check(keys, payload, key_bits, 0, SD.LARGE_CAPACITY, NO_RUNS, [SD.FORM_CHAINED_TILES] + ZERO_CENSUS)


@pytest.mark.parametrize('key_bits,cap_factor,big', [(9, 1, False), (15, 1, False), (31, 1, False), (41, 1, False),
                                                     (31, 3, False), (31, 1, True)])
def test_msd_partition_buckets(key_bits, cap_factor, big):
    """MSD partition + bucket_sort_kernel<true, 4096> (capacity = n; 0, 4, 20 and 30 key bits inside a bucket): buckets of
    0, 1, 2, 255 / 256 / 257, 4095 / 4096 / 4097 and 2^k, 2^k + 1 words, with one key, with distinct keys (4 key bits: every
    one of the 16 keys) in many small groups (two-level sort) and with one group so large that the rank cost is just above / just at or below 256 per word
    (LDS network / two-level sort; which of the two ran is the predictor's word alone - the census counts them together).
    Once in 3 n slots (stale words behind n)."""
    key_base = 77 << 40 if key_bits == 31 else 0
    _, keys, payload = SD.msd_stream(key_bits, key_base=key_base, big=big)
    want = SD.msd_census(SD.predict_msd(keys, key_bits, key_base))
    reduce_and_check(keys, payload, key_bits, key_base, cap_factor * len(keys), 0, want)


@pytest.mark.parametrize('one_chunk,big', [(False, False), (True, False), (False, True)])
def test_run_grouped_chunks(one_chunk, big):
    """The run-grouped form (4.3 M slots, no flag): chunks with exactly 63 and exactly 64 distinct keys, one key filling a
    chunk, a key whose only tuple is a chunk's last word, one key in every one of 200 chunks, a last chunk of one tuple;
    and a stream of exactly one chunk."""
    key_bits = 37
    keys, payload, _ = SD.runs_stream(key_bits, exactly_one_chunk=one_chunk, big=big)
    reduce_and_check(keys, payload, key_bits, 0, SD.LARGE_CAPACITY, 0, [SD.FORM_RUNS] + ZERO_CENSUS)
