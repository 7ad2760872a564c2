"""The designed streams of tests/sort_design.py hold every case they are meant to hold, and the predictors put each case
into the size class it was designed for.  No GPU: this is what keeps tests/test_gpu_sort_classes.py from quietly testing
something else than it names."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from tests import sort_design as SD

CHAINED_KEY_BITS = [25, 30, 37, 41]
MSD_KEY_BITS = [9, 15, 31, 41]


def bucket_lows(keys, key_base, low_bits, number):
    """The low keys of one designed bucket, in stream order."""
    rel = keys - np.uint64(key_base)
    mine = (rel >> np.uint64(low_bits)) == np.uint64(number)
    return (rel[mine] & np.uint64((1 << low_bits) - 1)).astype(np.int64)


def by_label(buckets, label):
    hit = [b for b in buckets if b.label == label]
    assert len(hit) == 1, label
    return hit[0]


def test_constants_mirror_the_build_knobs():
    for name, value in SD.source_knobs().items():
        assert getattr(SD, name) == value, name
    assert SD.run_chunk() % 64 == 0 and SD.run_chunk() >= 64
    # 1050 sort tiles: beyond the 1024 of the 4 M path
    assert -(-SD.LARGE_CAPACITY // 4096) > 1024 >= -(-(4 << 20) // 4096)


@pytest.mark.parametrize('key_bits', CHAINED_KEY_BITS)
def test_chained_cases_are_present_and_predicted(key_bits):
    low_bits = key_bits - SD.TOP_BITS
    key_base = (3 << 45) + 12_345 if key_bits in (30, 41) else 0
    buckets, keys, payload = SD.chained_stream(key_bits, key_base=key_base)
    assert len(keys) <= 400_000 and len(keys) == sum(c for b in buckets for _, c in b.keys)
    cls = SD.predict_chained(keys, key_bits, key_base)
    for b in buckets:
        assert cls[b.number] == b.want, '%s: predicted %s' % (b.label, SD.CHAINED_NAMES[cls[b.number]])
    designed = {b.number for b in buckets}
    assert all(cls[k] == SD.EMPTY for k in range(1 << SD.TOP_BITS) if k not in designed)
    labels = {b.label for b in buckets}
    # -- wave kernel
    sizes = [1, 2, 63, 64, 65] + [256 * k + d for k in range(1, 7) for d in (-1, 0, 1) if 256 * k + d <= 1536]
    assert 1535 in sizes and 1536 in sizes and 1281 in sizes
    for n in sizes:
        for k in (1, 2, 8, 48):
            if k <= n:
                b = by_label(buckets, 'wave n=%d keys=%d' % (n, k))
                assert sum(c for _, c in b.keys) == n and len(b.keys) == k and b.want == SD.WAVE
    b = by_label(buckets, 'wave low keys 0 and max')
    assert {k for k, _ in b.keys} == {0, (1 << low_bits) - 1}
    b = by_label(buckets, 'wave adjacent keys')
    assert b.keys[1][0] == b.keys[0][0] + 1
    b = by_label(buckets, 'wave key only in lane 0 of round 0')
    lows = bucket_lows(keys, key_base, low_bits, b.number)
    assert (lows == lows[0]).sum() == 1
    b = by_label(buckets, 'wave key only as the last word')
    lows = bucket_lows(keys, key_base, low_bits, b.number)
    assert (lows == lows[-1]).sum() == 1
    b = by_label(buckets, 'wave nine keys, eight smallest cover exactly a sixth')
    cnt = [c for _, c in sorted(b.keys)]
    assert len(cnt) == 9 and sum(cnt[:8]) * 6 == sum(cnt)
    b2 = by_label(buckets, 'digit nine keys, eight smallest cover one tuple less')
    cnt2 = [c for _, c in sorted(b2.keys)]
    assert len(cnt2) == 9 and sum(cnt2) == sum(cnt) and sum(cnt2[:8]) == sum(cnt[:8]) - 1 and b2.want == SD.WAVE_DIGIT
    # -- the wave kernel's digit passes
    assert len(by_label(buckets, 'digit 49 keys').keys) == 49
    assert max(len(b.keys) for b in buckets if b.want == SD.WAVE) == 48
    for n in (49, 64, 65, 1535, 1536):
        b = by_label(buckets, 'digit %s n=%d' % ('all-distinct' if n <= 1 << low_bits else 'every low key', n))
        assert sum(c for _, c in b.keys) == n and len(b.keys) == min(n, 1 << low_bits)
    for n in (200, 512, 1536):
        cnt = [c for _, c in sorted(by_label(buckets, 'digit long row between singletons n=%d' % n).keys)]
        assert cnt == [1] * 8 + [n - 16] + [1] * 8
        first, last = 8, 8 + n - 16 - 1                     # sorted places of the long row: it is carried over these rounds
        assert last // 64 - first // 64 + 1 >= 3 and (n < 1536 or last // 64 - first // 64 + 1 == 24)
    cnt = [c for _, c in sorted(by_label(buckets, 'digit rows of 64 and 128 ending on a round border').keys)]
    ends = np.cumsum(cnt)
    assert cnt[0] == 64 and cnt[1] == 128 and ends[0] % 64 == 0 and ends[1] % 64 == 0
    cnt = [c for _, c in sorted(by_label(buckets, 'digit row from lane 63 to a round border, single word in lane 0 behind it').keys)]
    starts = np.cumsum(cnt) - cnt
    assert starts[63] == 63 and cnt[63] > 1 and (starts[63] + cnt[63]) % 64 == 0 and cnt[64] == 1 and starts[64] % 64 == 0
    cnt = [c for _, c in sorted(by_label(buckets, 'digit row starting in lane 63').keys)]
    assert (np.cumsum(cnt) - cnt)[-1] == 63 and cnt[-1] > 1
    cnt = [c for _, c in sorted(by_label(buckets, 'digit carried row is the last').keys)]
    assert cnt[-1] > 64 and (sum(cnt) - 1) // 64 > (sum(cnt) - cnt[-1]) // 64
    lows = sorted(k for k, _ in by_label(buckets, 'digit keys that differ only in digit 0 / only in the top digit').keys)
    n_pass = -(-low_bits // SD.BK_DIGIT_BITS)
    top_shift = SD.BK_DIGIT_BITS * (n_pass - 1)
    same_high = [k for k in lows if k >> SD.BK_DIGIT_BITS == lows[len(lows) // 2] >> SD.BK_DIGIT_BITS]
    assert len(same_high) >= 50
    same_low = [k for k in lows if k & ((1 << top_shift) - 1) == 0x55]
    assert len(same_low) == min(1 << (low_bits - top_shift), 8) >= 2
    # -- workgroup kernel
    for n in (1537, 4095, 4096, 4097, 8192, 8193, 12_289, 20_000):
        one, many = by_label(buckets, 'workgroup n=%d one key' % n), by_label(buckets, 'workgroup n=%d ~300 keys' % n)
        assert len(one.keys) == 1 and len(many.keys) == min(300, 1 << low_bits)
        assert sum(c for _, c in one.keys) == n == sum(c for _, c in many.keys)
        assert one.want == many.want == (SD.WG_LDS if n <= 4096 else SD.WG_GLOBAL)
    assert len(by_label(buckets, 'workgroup n=4097 %s' % ('all-distinct' if low_bits >= 13 else 'every low key')).keys) == min(4097, 1 << low_bits)
    # -- the row mover's borders
    for number in (0, 1, 1023, 1024, 1025, 65_534, 65_535):
        assert 'row mover bucket %d' % number in labels and cls[number] == SD.WAVE
    # every arrangement is in use, and the interleaving kept the listed order
    assert {b.arrangement for b in buckets} == set(SD.ARRANGEMENTS)
    b = next(b for b in buckets if b.arrangement == 'descending' and len(b.keys) > 1)
    lows = bucket_lows(keys, key_base, low_bits, b.number)
    assert (np.diff(lows) <= 0).all() and lows[0] > lows[-1]
    # distinct observations: a row's observation order identifies its tuples
    assert len(np.unique(payload)) == len(payload)


def test_a_wrong_constant_is_named_by_the_census_message(monkeypatch):
    """The guard the GPU tests rely on: were the wave kernel's capacity 1280 and not 1536, the census of a designed stream
    would differ from the prediction and the message would name the classes."""
    buckets, keys, _ = SD.chained_stream(30)
    truth = SD.chained_census(SD.predict_chained(keys, 30))
    assert SD.explain_census(truth, truth) == ''
    monkeypatch.setattr(SD, 'WAVE_MAX_WORDS', 1280)
    wrong = SD.chained_census(SD.predict_chained(keys, 30))
    msg = SD.explain_census(truth, wrong)
    assert 'wave: ' in msg and 'workgroup in LDS: ' in msg and 'predicted' in msg
    assert 'form' in SD.explain_census([1] + [0] * 7, truth)


@pytest.mark.parametrize('key_bits', [20, 45])
def test_tile_rows_sit_on_the_tile_borders(key_bits):
    T = SD.RED_TILE
    keys, payload = SD.tile_stream(key_bits)
    assert int(keys.max()).bit_length() <= key_bits and (np.diff(keys.astype(np.int64)) < 0).any()
    starts, cnt = SD.row_starts(keys)
    offs = set((starts % T).tolist())
    assert {0, 1, T - 1} <= offs
    assert any(s % T == 0 and c == T for s, c in zip(starts, cnt))
    assert any(s % T == 0 and c == 2 * T for s, c in zip(starts, cnt))
    assert any(s % T == 0 and c == 2 * T + 1 for s, c in zip(starts, cnt))
    assert any(s == T // 2 and s + c == 5 * T + T // 2 for s, c in zip(starts, cnt))
    assert not set(range(1, 5)) & set((starts // T).tolist())         # tiles without any head
    assert len(keys) % T == 0 and 40_000 < len(keys) < 50_000
    more, _ = SD.tile_stream(key_bits, one_more=True)
    assert len(more) % T == 1 and len(SD.row_starts(more)[0]) == len(starts)


@pytest.mark.parametrize('key_bits', MSD_KEY_BITS)
def test_msd_cases_are_present_and_predicted(key_bits):
    sub_bits = max(key_bits - SD.MSD_BITS, 0)
    key_base = 77 << 40 if key_bits == 31 else 0
    buckets, keys, payload = SD.msd_stream(key_bits, key_base=key_base)
    assert len(keys) <= 400_000
    cls = SD.predict_msd(keys, key_bits, key_base)
    for b in buckets:
        assert cls[b.number] == b.want, '%s: predicted %s' % (b.label, SD.MSD_NAMES[cls[b.number]])
    assert cls[5] == SD.MSD_LE1 and 5 not in {b.number for b in buckets}          # a bucket of size 0
    want_sizes = {1, 2, 255, 256, 257, 4095, 4096, 4097, 512, 513, 8192, 8193}
    assert {sum(c for _, c in b.keys) for b in buckets if b.label.endswith('one key')} == want_sizes
    if sub_bits:
        assert {sum(c for _, c in b.keys) for b in buckets if 'many small groups' in b.label} == want_sizes - {1}
        for n in (257, 512, 513, 4095, 4096):
            above = by_label(buckets, 'msd n=%d one large group, cost just above the limit' % n)
            assert above.want == SD.MSD_LDS_NETWORK and sum(c for _, c in above.keys) == n
            below = by_label(buckets, 'msd n=%d one large group, cost just at or below the limit' % n)
            assert below.want == SD.MSD_TWO_LEVEL and sum(c for _, c in below.keys) == n
            # neighbours: one word moved into the large group crosses the limit
            big = lambda b: max(np.bincount([k >> max(sub_bits - 8, 0) for k, _ in b.keys], weights=[c for _, c in b.keys]))
            assert big(above) == big(below) + 1
        assert {SD.MSD_LE1, SD.MSD_RANK, SD.MSD_TWO_LEVEL, SD.MSD_LDS_NETWORK, SD.MSD_GLOBAL_NETWORK} == {b.want for b in buckets}
    for n in want_sizes - {1} if sub_bits else ():
        b = by_label(buckets, 'msd n=%d %s keys, many small groups' % (n, 'all-distinct' if n <= 1 << sub_bits else 'every low key'))
        assert len(b.keys) == min(n, 1 << sub_bits)


def test_run_chunks_are_designed_on_the_chunk_borders():
    chunk = SD.run_chunk()
    keys, payload, shared = SD.runs_stream(37)
    prof = SD.chunk_profile(keys, chunk)
    assert len(keys) <= 400_000 and len(keys) % chunk == 1 and prof[-1] == 1
    assert prof[0] == 63 and prof[1] == 64 and prof[2] == 1
    last = keys[4 * chunk - 1]
    assert (keys == last).sum() == 1
    with_shared = [i for i in range(len(prof)) if (keys[i * chunk:(i + 1) * chunk] == np.uint64(shared)).any()]
    assert len(with_shared) == SD.RUN_SHARED_CHUNKS == 200
    one, _, _ = SD.runs_stream(37, exactly_one_chunk=True)
    assert len(one) == chunk


def test_magnitudes_stay_inside_the_oracles_int64():
    """Large observations: drawn from [2^24, 2^25) (rows of up to 1024 tuples) and [2^19, 2^20) (longer rows): squares beyond
    2^32 everywhere, sums beyond 2^32, and nothing the numpy oracle's int64 could wrap on."""
    buckets, keys, payload = SD.chained_stream(37, big=True)
    rows = CO.edge_rows(keys, payload)
    o = rows['obs_lo'] + rows['obs_hi']
    assert o.min() >= 1 << 20 and o.max() < 1 << 26 and (o >= 1 << 25).any()
    exact_sq = [sum(int(v) ** 2 for v in o[s:s + c]) for s, c in zip(rows['offset'][:50], rows['n'][:50])]
    assert exact_sq == rows['sum_obs_sq'][:50].tolist()
    assert rows['sum_obs_sq'].max() < 1 << 63 and rows['sum_obs_sq'].max() > 1 << 56
    five = rows['n'] == 5000
    assert five.sum() == 1 and rows['sum_obs'][five][0] > 1 << 32
    for keys, payload in (SD.tile_stream(20, big=True), SD.msd_stream(31, big=True)[1:], SD.runs_stream(37, big=True)[:2]):
        rows = CO.edge_rows(keys, payload)
        assert (rows['sum_obs_sq'] > 1 << 40).all() and rows['sum_obs_sq'].max() < 1 << 63
        assert rows['sum_obs'].max() > 1 << 32
