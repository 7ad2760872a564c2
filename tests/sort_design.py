"""Designed tuple streams for stage 2 (csrc/sortreduce.hip, onesweep.hip, runs.hip) and a prediction of the kernel that
finishes each of their buckets.  Plain numpy; nothing here is imported from, or computed by, the kernels under test.

Stage 2 picks its kernels per bucket, by the bucket's size and key structure.  A drawn stream meets the borders of those
size classes by accident; the streams below place a bucket on each side of every border on purpose, and the predictors
say - from the rules as the sources state them - which class each bucket is meant for.  tests/test_sort_design.py
checks, without a GPU, that every designed case is in its stream and predicted into its class; the GPU tests then hold
besst_dev_reduce_census (what the call really did) against the same prediction.

A stream is built from designed buckets: (bucket number, [(low key, count), ...], arrangement).  A key is
(bucket << low_bits) | low (+ key_base); the tuples of all buckets are interleaved by a seeded permutation that keeps
every bucket's own arrangement."""
import collections
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'besst_amd', 'csrc')

# ---- the dispatch constants, each with the build knob or source line it mirrors ------------------------------------
TOP_BITS = 16              # onesweep.hip kTopBuckets = 1 << 16: the bucket form's stream passes sort the top 16 bits
WAVE_MAX_WORDS = 1536      # onesweep.hip kBwCap = 64 * BESST_BW_ITEMS (24): largest bucket of the wave kernels
WAVE_TEMPLATE_STEP = 256   # os_bucket_wave_kernel: templates of 4, 8, .. rounds of 64, picked by (n + 255) >> 8
WAVE_MAX_KEYS = 48         # BESST_BW_KEYS: a 49th distinct key sends the bucket to the digit passes
WAVE_COVER_KEYS = 8        # bw_bucket, `K == 8 && covered * 6u < n`: from the ninth key on, the eight smallest keys ...
WAVE_COVER_DIV = 6         # ... must cover at least a sixth of the bucket
WG_LDS_WORDS = 4096        # onesweep.hip kBkCap = kBkThreads * kBkItems: os_bucket_sort_kernel sorts in LDS up to here
BK_DIGIT_BITS = 7          # BESST_BK_BITS: digit width of the bucket kernels' passes
MSD_BITS = 11              # BESST_MSD_BITS: the partition digit of the form for up to 4 M slots
RANK_MAX = 256             # sortreduce.hip bucket_rank_max(4096): plain rank sort up to here
MSD_LDS_WORDS = 4096       # sortreduce.hip kBucketPackedCap: two-level sort / LDS network up to here
RANK_COST_LIMIT = 256      # BESST_RANK_COST_LIMIT: sum of squared group sizes > 256 * n -> the LDS bitonic network
GROUP_BITS = 8             # bucket_sort_kernel: the two-level sort groups by the next 8 key bits
RED_TILE = 4096            # onesweep.hip kOsRedTile: tile of os_reduce_kernel
ROW_MOVER_BUCKETS = 1024   # onesweep.hip kRowsThreads: buckets per workgroup of os_bucket_rows_kernel

LARGE_CAPACITY = 4_300_000  # 1050 sort tiles of 4096: the smallest capacity that leaves the 4 M path (1024 tiles) by a margin

# classes of a top-16-bit bucket (chained scan + buckets), in the order besst_dev_reduce_census counts them
EMPTY, WAVE, WAVE_DIGIT, WG_LDS, WG_GLOBAL = range(5)
CHAINED_NAMES = ['empty', 'wave', 'wave digit passes', 'workgroup in LDS', 'workgroup in global memory']
# classes of an 11-bit bucket (MSD partition + buckets)
MSD_LE1, MSD_RANK, MSD_TWO_LEVEL, MSD_LDS_NETWORK, MSD_GLOBAL_NETWORK = range(5)
MSD_NAMES = ['<= 1 word', 'rank sort', 'two-level sort', 'LDS network', 'global network']
MSD_CENSUS_NAMES = ['<= 1 word', '2..256 words', '257..4096 words', '> 4096 words']

FORM_MSD, FORM_RUNS, FORM_CHAINED_BUCKETS, FORM_CHAINED_TILES = range(4)


def _knob(source, name):
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(r'#define\s+%s\s+(\d+)' % re.escape(name), text)
    assert m, '%s: no default for %s' % (source, name)
    return int(m.group(1))


def run_chunk():
    """Tuples per chunk of the run-grouped form: kRunChunk = 64 * BESST_RG_ROUNDS, read from csrc/common.h (the one place
    that defines it)."""
    return 64 * _knob('common.h', 'BESST_RG_ROUNDS')


def source_knobs():
    """The build knobs' defaults as the sources have them, keyed like the constants above (for the CPU test)."""
    return dict(WAVE_MAX_WORDS=64 * _knob('onesweep.hip', 'BESST_BW_ITEMS'), WAVE_MAX_KEYS=_knob('onesweep.hip', 'BESST_BW_KEYS'),
                BK_DIGIT_BITS=_knob('onesweep.hip', 'BESST_BK_BITS'), MSD_BITS=_knob('sortreduce.hip', 'BESST_MSD_BITS'),
                RANK_COST_LIMIT=_knob('sortreduce.hip', 'BESST_RANK_COST_LIMIT'))


# ---- predictors ------------------------------------------------------------------------------------------------------
def _buckets_of(keys, key_bits, key_base, bucket_bits):
    """-> {bucket: (sorted distinct low keys, their counts)} of key - key_base split at key_bits - bucket_bits."""
    rel = np.asarray(keys, dtype=np.uint64) - np.uint64(key_base)
    assert len(rel) == 0 or int(rel.max()).bit_length() <= key_bits, 'a key does not fit key_bits'
    low_bits = max(key_bits - bucket_bits, 0)
    uniq, cnt = np.unique(rel, return_counts=True)
    bucket = (uniq >> np.uint64(low_bits)).astype(np.int64)
    low = (uniq & np.uint64((1 << low_bits) - 1)).astype(np.int64)
    out = {}
    edges = np.nonzero(np.diff(bucket))[0] + 1
    for lo, hi in zip(np.concatenate(([0], edges)), np.concatenate((edges, [len(uniq)]))):
        if hi > lo:
            out[int(bucket[lo])] = (low[lo:hi], cnt[lo:hi].astype(np.int64))
    return out


def chained_class(counts):
    """The kernel that finishes a top-16-bit bucket whose distinct keys, in rising order, hold `counts` tuples."""
    n, k = int(np.sum(counts)), len(counts)
    if n == 0:
        return EMPTY
    if n > WAVE_MAX_WORDS:
        return WG_LDS if n <= WG_LDS_WORDS else WG_GLOBAL
    if k > WAVE_MAX_KEYS:
        return WAVE_DIGIT
    if k > WAVE_COVER_KEYS and int(np.sum(counts[:WAVE_COVER_KEYS])) * WAVE_COVER_DIV < n:
        return WAVE_DIGIT
    return WAVE


def predict_chained(keys, key_bits, key_base=0):
    """Class of every top-16-bit bucket of the chained scan + buckets form -> int array of 1 << 16."""
    cls = np.full(1 << TOP_BITS, EMPTY, dtype=np.int64)
    for b, (low, cnt) in _buckets_of(keys, key_bits, key_base, TOP_BITS).items():
        cls[b] = chained_class(cnt)
    return cls


def msd_class(low, counts, sub_bits):
    """The branch of bucket_sort_kernel<true, 4096> a bucket takes: `low` its distinct keys below the partition digit
    (sub_bits of them), `counts` their tuples."""
    n = int(np.sum(counts))
    if n <= 1:
        return MSD_LE1
    if n <= RANK_MAX:
        return MSD_RANK
    if n > MSD_LDS_WORDS:
        return MSD_GLOBAL_NETWORK
    group = (low >> (sub_bits - GROUP_BITS)) if sub_bits >= GROUP_BITS else (low & ((1 << sub_bits) - 1))
    size = np.bincount(group, weights=counts, minlength=1).astype(np.int64)
    cost = int(np.sum(size[size > 1] ** 2))
    return MSD_LDS_NETWORK if cost > RANK_COST_LIMIT * n else MSD_TWO_LEVEL


def predict_msd(keys, key_bits, key_base=0):
    """Class of every 11-bit bucket of the MSD partition + buckets form -> int array of 1 << 11."""
    cls = np.full(1 << MSD_BITS, MSD_LE1, dtype=np.int64)
    sub_bits = max(key_bits - MSD_BITS, 0)
    for b, (low, cnt) in _buckets_of(keys, key_bits, key_base, MSD_BITS).items():
        cls[b] = msd_class(low, cnt, sub_bits)
    return cls


def chained_census(cls):
    """What besst_dev_reduce_census reports for form 2: [form, empty, wave, digit passes, LDS, global, 0, 0]."""
    return [FORM_CHAINED_BUCKETS] + [int((cls == c).sum()) for c in range(5)] + [0, 0]


def msd_census(cls):
    """... and for form 0: the census cannot tell the two-level sort from the LDS network (both 257..4096 words)."""
    c = [int((cls == k).sum()) for k in range(5)]
    return [FORM_MSD, c[0], c[1], c[2] + c[3], c[4], 0, 0, 0]


def explain_census(got, want):
    """'' when equal, else a message that names the classes that differ."""
    if list(got) == list(want):
        return ''
    if got[0] != want[0]:
        return 'stage 2 took form %d, the stream was designed for form %d' % (got[0], want[0])
    names = CHAINED_NAMES if want[0] == FORM_CHAINED_BUCKETS else MSD_CENSUS_NAMES
    diff = ['%s: %d buckets, predicted %d' % (names[k], got[1 + k], want[1 + k]) for k in range(len(names))
            if got[1 + k] != want[1 + k]]
    return 'bucket classes differ from the prediction - ' + '; '.join(diff)


# ---- designed buckets -> stream ----------------------------------------------------------------------------------------
# label: what the case is there for; want: the class it is designed for (None: not a bucket-class case)
Bucket = collections.namedtuple('Bucket', 'number keys arrangement label want')

ARRANGEMENTS = ('shuffled', 'descending', 'listed', 'first_last')


def _arrange(keys, arrangement, rng):
    """The bucket's low keys, one per tuple, in the bucket's own order.
    shuffled; descending (falling keys: the sort really permutes); listed (as given); first_last: shuffled, but the
    LAST listed key's tuples come behind all others - with a count of 1 its first tuple is the bucket's last word."""
    low = np.repeat(np.array([k for k, _ in keys], dtype=np.int64), [c for _, c in keys])
    if arrangement == 'listed':
        return low
    if arrangement == 'descending':
        return np.sort(low)[::-1].copy()
    if arrangement == 'shuffled':
        return rng.permutation(low)
    assert arrangement == 'first_last', arrangement
    tail = keys[-1][1]
    return np.concatenate((rng.permutation(low[:len(low) - tail]), low[len(low) - tail:]))


def distinct_obs(rng, n, lo, hi):
    """n pairwise different (obs1, obs2) pairs, both in [lo, hi) (lo and hi may be arrays: a range per tuple)."""
    lo = np.broadcast_to(np.asarray(lo, dtype=np.int64), (n,))
    span = np.broadcast_to(np.asarray(hi, dtype=np.int64), (n,)) - lo
    code = (rng.random(n) * (span * span)).astype(np.int64)
    for _ in range(64):
        a, b = lo + code // span, lo + code % span
        _, first = np.unique((a << 32) | b, return_index=True)
        dup = np.ones(n, bool)
        dup[first] = False
        if not dup.any():
            return a, b
        code[dup] = (rng.random(int(dup.sum())) * (span[dup] * span[dup])).astype(np.int64)
    raise AssertionError('could not draw distinct observations')


SMALL_OBS = (26, 5000)                  # what every earlier sort-stage test draws from
BIG_OBS = (1 << 24, 1 << 25)            # o1 + o2 < 2^26: squares up to 2^52
LONG_ROW_OBS = (1 << 19, 1 << 20)       # rows of more than BIG_ROW_MAX tuples: o1 + o2 < 2^21, 20 000 * 2^42 < 2^63
BIG_ROW_MAX = 1024                      # 1024 * 2^52 = 2^62


def make_payload(keys, rng, big=False):
    """Payload words for `keys`: distinct random observations (a row's observation order then proves stability), the graph
    mask a function of the key.  big: large magnitudes - rows of up to 1024 tuples draw from BIG_OBS, longer
    ones from LONG_ROW_OBS; the bounds that keep the int64 oracle from wrapping are asserted."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    if not big:
        lo_v, hi_v = distinct_obs(rng, n, SMALL_OBS[0], SMALL_OBS[1])
        bound = n * (2 * (SMALL_OBS[1] - 1)) ** 2
    else:
        _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
        long_row = cnt[inv] > BIG_ROW_MAX
        top = np.where(long_row, LONG_ROW_OBS[1], BIG_OBS[1]).astype(np.int64)
        base = np.where(long_row, LONG_ROW_OBS[0], BIG_OBS[0]).astype(np.int64)
        lo_v, hi_v = distinct_obs(rng, n, base, top)
        short, long_ = cnt[cnt <= BIG_ROW_MAX], cnt[cnt > BIG_ROW_MAX]
        bound = max(int(short.max(initial=0)) * (2 * (BIG_OBS[1] - 1)) ** 2, int(long_.max(initial=0)) * (2 * (LONG_ROW_OBS[1] - 1)) ** 2)
    assert bound < 1 << 63, 'a row sum of squares could wrap int64'
    assert n == 0 or (int(lo_v.max()) + int(hi_v.max()) < 1 << 30 and int(hi_v.max()) < 1 << 30 and int(lo_v.min()) >= 0)
    mask = (keys >> np.uint64(1)) % np.uint64(3) + np.uint64(1)
    return lo_v.astype(np.uint64) | ((hi_v.astype(np.uint64) | (mask << np.uint64(30))) << np.uint64(32))


def build_stream(buckets, low_bits, seed, key_base=0, big=False):
    """(keys, payload) of the designed buckets, interleaved by a seeded permutation that keeps each bucket's arrangement."""
    rng = np.random.default_rng(seed)
    numbers = [b.number for b in buckets]
    assert len(set(numbers)) == len(numbers), 'two designed buckets share a number'
    parts = []
    for b in buckets:
        lows = [k for k, _ in b.keys]
        assert len(set(lows)) == len(lows) and all(0 <= k < 1 << low_bits and c >= 1 for k, c in b.keys), b.label
        parts.append((np.int64(b.number) << low_bits) | _arrange(b.keys, b.arrangement, rng))
    sizes = [len(p) for p in parts]
    owner = rng.permutation(np.repeat(np.arange(len(parts)), sizes))
    keys = np.empty(len(owner), dtype=np.int64)
    for j, p in enumerate(parts):
        keys[owner == j] = p
    keys = keys.astype(np.uint64) + np.uint64(key_base)
    return keys, make_payload(keys, rng, big)


def spread_lows(k, low_bits):
    """k distinct low keys spread over [0, 2^low_bits), rising."""
    top = 1 << low_bits
    assert k <= top
    if k == top:
        return list(range(top))
    step = top // k
    return [j * step + (step // 3 if step > 2 else 0) for j in range(k)]


def distinct_label(n, space):
    """How a case of n tuples that asks for n distinct keys is labelled when only `space` keys exist: it then holds every
    one of them, several tuples each."""
    return 'all-distinct' if n <= space else 'every low key'


def front_loaded(n, k):
    """n tuples over k keys as evenly as possible, the remainder on the SMALLEST keys (so the eight smallest of 48 keys
    always cover a sixth)."""
    q, r = divmod(n, k)
    return [q + (1 if j < r else 0) for j in range(k)]


WAVE_SIZES = [1, 2, 63, 64, 65] + [WAVE_TEMPLATE_STEP * k + d for k in range(1, 7) for d in (-1, 0, 1)
                                   if WAVE_TEMPLATE_STEP * k + d <= WAVE_MAX_WORDS]
WG_SIZES = [1537, 4095, 4096, 4097, 8192, 8193, 12_289, 20_000]
ROW_MOVER_NUMBERS = [0, 1, 1023, 1024, 1025, 65_534, 65_535]


def chained_cases(low_bits, extra_long_row=False):
    """The designed buckets of the chained scan + buckets form for keys of 16 + low_bits bits -> list of Bucket (numbers assigned here).
    Where a case asks for more distinct keys than 2^low_bits (all-distinct keys at low_bits 9), every low key is present
    and the tuples are dealt over them evenly."""
    top = 1 << low_bits
    cases = []                                               # (keys, arrangement, label, want)
    arr = lambda: ARRANGEMENTS[len(cases) % 3]               # shuffled / descending / listed in turn

    def add(keys, arrangement, label, want):
        cases.append((keys, arrangement, label, want))

    def distinct(n):
        k = min(n, top)
        return list(zip(spread_lows(k, low_bits), front_loaded(n, k)))

    # -- wave kernel: sizes at the template borders, 1 / 2 / 8 / 48 distinct keys
    for n in WAVE_SIZES:
        for k in (1, 2, 8, 48):
            if k <= n:
                add(list(zip(spread_lows(k, low_bits), front_loaded(n, k))), arr(), 'wave n=%d keys=%d' % (n, k), WAVE)
    add([(0, 100), (top - 1, 100)], 'shuffled', 'wave low keys 0 and max', WAVE)
    f = top // 2 - 1
    add([(f, 90), (f + 1, 110)], 'shuffled', 'wave adjacent keys', WAVE)
    add([(top // 2, 1), (5, 130), (top - 3, 69)], 'listed', 'wave key only in lane 0 of round 0', WAVE)
    add([(5, 130), (top - 3, 69), (top // 2, 1)], 'first_last', 'wave key only as the last word', WAVE)
    nine = spread_lows(9, low_bits)
    add(list(zip(nine, [10] * 8 + [400])), 'shuffled', 'wave nine keys, eight smallest cover exactly a sixth', WAVE)
    add(list(zip(nine, [10] * 7 + [9, 401])), 'shuffled', 'digit nine keys, eight smallest cover one tuple less', WAVE_DIGIT)
    # -- wave digit passes
    lows49 = spread_lows(49, low_bits)
    add(list(zip(lows49, [20] * 8 + [5] * 41)), 'shuffled', 'digit 49 keys', WAVE_DIGIT)
    for n in (49, 64, 65, 1535, 1536):
        add(distinct(n), arr(), 'digit %s n=%d' % (distinct_label(n, top), n), WAVE_DIGIT)
    for n in (200, 512, 1536):
        lows = spread_lows(17, low_bits)
        add(list(zip(lows, [1] * 8 + [n - 16] + [1] * 8)), 'descending' if n == 512 else 'shuffled',
            'digit long row between singletons n=%d' % n, WAVE_DIGIT)
    lows = spread_lows(50, low_bits)
    add(list(zip(lows, [64, 128] + [1] * 48)), 'shuffled', 'digit rows of 64 and 128 ending on a round border', WAVE_DIGIT)
    lows = spread_lows(65, low_bits)
    add(list(zip(lows, [1] * 63 + [65, 1])), 'shuffled',
        'digit row from lane 63 to a round border, single word in lane 0 behind it', WAVE_DIGIT)
    lows = spread_lows(64, low_bits)
    add(list(zip(lows, [1] * 63 + [10])), 'descending', 'digit row starting in lane 63', WAVE_DIGIT)
    lows = spread_lows(61, low_bits)
    add(list(zip(lows, [1] * 60 + [100])), 'shuffled', 'digit carried row is the last', WAVE_DIGIT)
    n_pass = (low_bits + BK_DIGIT_BITS - 1) // BK_DIGIT_BITS
    shift = BK_DIGIT_BITS * (n_pass - 1)
    digit0 = [(1 << shift) | d for d in range(50)] if shift else list(range(50))
    tops = [(t << shift) | 0x55 for t in range(min(1 << (low_bits - shift), 8))]
    assert not set(digit0) & set(tops)
    add([(k, 2) for k in sorted(digit0 + tops)], 'shuffled', 'digit keys that differ only in digit 0 / only in the top digit',
        WAVE_DIGIT)
    # -- workgroup kernel
    for n in WG_SIZES:
        want = WG_LDS if n <= WG_LDS_WORDS else WG_GLOBAL
        add([(top // 3, n)], 'listed', 'workgroup n=%d one key' % n, want)
        k = min(300, top)
        add(list(zip(spread_lows(k, low_bits), front_loaded(n, k))), arr(), 'workgroup n=%d ~300 keys' % n, want)
    add(distinct(4097), 'shuffled', 'workgroup n=4097 %s' % distinct_label(4097, top), WG_GLOBAL)
    if extra_long_row:
        add([(top // 5, 5000)], 'listed', 'workgroup one row of 5000 tuples (sum beyond 2^32)', WG_GLOBAL)
    # -- numbers: the designed buckets spread over the whole range, the row mover's borders kept for its own copies
    stride = ((1 << TOP_BITS) - 3000) // len(cases)
    out = [Bucket(1500 + j * stride, *c) for j, c in enumerate(cases)]
    small = [(3, 7), (top // 2, 30), (top - 1, 2)]
    out += [Bucket(b, small, 'shuffled', 'row mover bucket %d' % b, WAVE) for b in ROW_MOVER_NUMBERS]
    assert not {b.number for b in out[:len(cases)]} & set(ROW_MOVER_NUMBERS)
    return out


def chained_stream(key_bits, seed=0, key_base=0, big=False):
    buckets = chained_cases(key_bits - TOP_BITS, extra_long_row=big)
    keys, payload = build_stream(buckets, key_bits - TOP_BITS, seed + key_bits, key_base, big)
    return buckets, keys, payload


def tiny_stream(n, key_bits, seed=0):
    """A nearly empty stream: n tuples over about n / 3 random keys."""
    rng = np.random.default_rng(seed + n)
    pool = rng.integers(0, 1 << key_bits, max(1, n // 3), dtype=np.int64)
    keys = pool[rng.integers(0, len(pool), n)].astype(np.uint64)
    return keys, make_payload(keys, rng)


# ---- chained scan + tile reduction: rows placed against the 4096-tuple tiles ---------------------------------------------
T = RED_TILE
TILE_ROW_STARTS = [0, 1, T // 2, 5 * T + T // 2, 5 * T + T - 1, 6 * T, 7 * T, 9 * T, 11 * T + 1,
                   11 * T + 8, 11 * T + 72, 11 * T + 172, 11 * T + 1172, 11 * T + 2072]
TILE_STREAM_END = 12 * T


def tile_stream(key_bits, seed=0, one_more=False, big=False):
    """Row k has key k * step and the length that puts the NEXT row's head at TILE_ROW_STARTS[k + 1] after the sort; the
    stream order is shuffled.  one_more: the last row runs one tuple into the next tile."""
    rng = np.random.default_rng(seed + key_bits + (1 if one_more else 0))
    ends = TILE_ROW_STARTS[1:] + [TILE_STREAM_END + (1 if one_more else 0)]
    lengths = np.array(ends) - np.array(TILE_ROW_STARTS)
    step = ((1 << key_bits) - 1) // (len(lengths) - 1)
    keys = rng.permutation(np.repeat(np.arange(len(lengths), dtype=np.int64) * step, lengths)).astype(np.uint64)
    return keys, make_payload(keys, rng, big)


def row_starts(keys):
    """Where each row begins in the sorted stream, and the rows' lengths."""
    _, cnt = np.unique(keys, return_counts=True)
    return np.cumsum(cnt) - cnt, cnt


# ---- MSD partition + buckets ----------------------------------------------------------------------------------------------
MSD_SIZES = sorted({1, 2, 255, 256, 257, 4095, 4096, 4097} | {(1 << k) + d for k in (9, 12, 13) for d in (0, 1)})


def _group_cost(sizes):
    s = np.array(sizes, dtype=np.int64)
    return int(np.sum(s[s > 1] ** 2))


def _skewed_groups(n, groups, above):
    """Group sizes for n words over `groups` (> 1) groups, one group holding most: the smallest large group whose cost
    (sum of squared sizes of the groups of more than one word) is above RANK_COST_LIMIT * n, or - above False - one word
    less in it, the nearest split at or below the limit (None when even the even split is above it)."""
    def sizes(g):
        return [g] + [r for r in front_loaded(n - g, groups - 1) if r]
    even = -(-n // groups)
    for g in range(even, n + 1):
        if _group_cost(sizes(g)) > RANK_COST_LIMIT * n:
            if above:
                return sizes(g)
            return sizes(g - 1) if g > even else None
    return None


def msd_cases(key_bits):
    """Designed buckets of the MSD partition + buckets form for key_bits-bit keys (sub_bits = key_bits - 11 key bits inside a bucket).
    Bucket number 5 stays empty (size 0)."""
    sub_bits = max(key_bits - MSD_BITS, 0)
    n_buckets = 1 << min(key_bits, MSD_BITS)
    sub_top = 1 << sub_bits
    group_shift = max(sub_bits - GROUP_BITS, 0)
    n_groups = 1 << min(sub_bits, GROUP_BITS)
    per_group = 1 << group_shift
    cases = []

    def add(keys, label, want):
        cases.append((keys, ARRANGEMENTS[len(cases) % 2], label, want))      # shuffled / descending

    def klass(n, mid):
        return MSD_LE1 if n <= 1 else MSD_RANK if n <= RANK_MAX else mid if n <= MSD_LDS_WORDS else MSD_GLOBAL_NETWORK

    def grouped(sizes):
        """Distinct keys where the group space allows, group j holding sizes[j] words."""
        keys = []
        gids = spread_lows(len(sizes), min(sub_bits, GROUP_BITS))
        for gid, size in zip(gids, sizes):
            k = min(size, per_group)
            keys += [((gid << group_shift) | low, c) for low, c in zip(spread_lows(k, group_shift), front_loaded(size, k))]
        return keys

    for n in MSD_SIZES:
        add([(sub_top // 2, n)], 'msd n=%d one key' % n, klass(n, MSD_LDS_NETWORK))     # one group of n: cost n^2 > 256 n
        if sub_bits == 0 or n == 1:
            continue
        k = min(n, sub_top)
        sizes = front_loaded(n, min(k, n_groups))
        mid = MSD_LDS_NETWORK if _group_cost(sizes) > RANK_COST_LIMIT * n else MSD_TWO_LEVEL
        add(grouped(sizes), 'msd n=%d %s keys, many small groups' % (n, distinct_label(n, sub_top)), klass(n, mid))
        if RANK_MAX < n <= MSD_LDS_WORDS and n_groups > 1:
            for above in (True, False):
                sizes = _skewed_groups(n, n_groups, above)
                if sizes is not None:
                    add(grouped(sizes), 'msd n=%d one large group, cost just %s the limit' % (n, 'above' if above else 'at or below'),
                        MSD_LDS_NETWORK if above else MSD_TWO_LEVEL)
    numbers = [b for b in range(n_buckets) if b != 5]
    stride = max(1, len(numbers) // len(cases))
    assert stride * (len(cases) - 1) < len(numbers), 'more cases than buckets'
    return [Bucket(numbers[j * stride], *c) for j, c in enumerate(cases)]


def msd_stream(key_bits, seed=0, key_base=0, big=False):
    buckets = msd_cases(key_bits)
    keys, payload = build_stream(buckets, max(key_bits - MSD_BITS, 0), seed + key_bits, key_base, big)
    return buckets, keys, payload


# ---- run-grouped form: chunks designed on the chunk borders ---------------------------------------------------------------
RUN_CHUNK_CASES = ['63 keys', '64 keys', 'one key', 'last word only']
RUN_SHARED_CHUNKS = 200


def runs_stream(key_bits, seed=0, exactly_one_chunk=False, big=False):
    """Chunks of run_chunk() tuples, in this order: exactly 63 distinct keys; exactly 64; one key filling the chunk; a key
    whose only tuple is the chunk's last word; 200 chunks that all hold the key SHARED (one row from 200 runs) among a few
    keys of their own; a last chunk of one tuple.  exactly_one_chunk: only the first of them (n = the chunk size)."""
    chunk = run_chunk()
    rng = np.random.default_rng(seed + key_bits)
    pool = rng.permutation(np.unique(rng.integers(0, 1 << (key_bits - 2), 5000, dtype=np.int64))) << 1   # distinct; SHARED is none of them
    shared = np.int64((1 << (key_bits - 1)) + 2)
    take = iter(pool)
    fresh = lambda k: np.array([next(take) for _ in range(k)], dtype=np.int64)

    def filled(keys_, n):
        return rng.permutation(np.repeat(keys_, front_loaded(n, len(keys_))))

    chunks = [filled(fresh(63), chunk)]
    if not exactly_one_chunk:
        chunks.append(filled(fresh(64), chunk))
        chunks.append(np.repeat(fresh(1), chunk))
        chunks.append(np.concatenate((filled(fresh(5), chunk - 1), fresh(1))))
        for _ in range(RUN_SHARED_CHUNKS):
            own = filled(fresh(6), chunk - 3)
            c = np.concatenate((own, np.repeat(shared, 3)))
            chunks.append(rng.permutation(c))
        chunks.append(fresh(1))
    keys = np.concatenate(chunks).astype(np.uint64)
    return keys, make_payload(keys, rng, big), int(shared)


def chunk_profile(keys, chunk):
    """Distinct keys of every chunk of `chunk` consecutive tuples."""
    return [len(np.unique(keys[i:i + chunk])) for i in range(0, len(keys), chunk)]
