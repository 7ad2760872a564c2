"""Designed inputs for the multi-GPU exchange (csrc/sortreduce.hip: partition_scatter_kernel behind radix_hist_kernel /
radix_rowscan_kernel in owner mode, and unpack_kernel), a plain model of both stages, a census of the structural borders
every design meets, and named WRONG models.  Plain numpy / Python; nothing here is imported from, or computed by, the
kernels under test.

An exchange is `world` sources; each source holds an ordered tuple stream (keys, payload, *n_tuples, capacity), an
optional rider and an optional slice description (speculative heads).  `partition` says what a source's send buffer must
hold, region by region; `unpack` says what a receiver makes of the regions the sources sent it.  The drawn workloads of
tests/test_gpu_distributed_sim.py meet the borders of these two stages by accident or never; the designs below place an
owner change on every lane, round, wave and tile border, a capacity on each side of the two switches between the three
forms of the partition, a region's total on each side of pair_capacity, the world at 1 and at 256, and the head replay
in every state of its flags.  tests/test_exchange_design.py checks all of that without a GPU;
tests/test_gpu_exchange_borders.py holds the kernels against the model with ==.

The head replay (`create_edge`) restates the CreateEdge call sequence of one record, oracle/py_oracle.py:511-530
(CreateGraph.py:176-183, 812-871): the first call against the running previous observations, the optional second call
against (-1, -1), the early return on a duplicate with detect_duplicate."""
import collections
import functools
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'besst_amd', 'csrc')
CANARY = 0xA5                                    # every byte of a send buffer before the first call
HEADER_BYTES = 64
HASH = 2654435761


# ---- the form constants, read from the sources -------------------------------------------------------------------------
def _knob(source, name):
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(r'#define\s+%s\s+(\d+)' % re.escape(name), text)
    assert m, '%s: no default for %s' % (source, name)
    return int(m.group(1))


def _const(source, pattern):
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(pattern, text)
    assert m, '%s: nothing matches %s' % (source, pattern)
    return int(m.group(1))


def source_knobs():
    """What picks the form of partition_scatter_kernel (launch_partition) and its geometry."""
    return dict(
        SCAN_FREE_MAX_BLOCKS=_knob('sortreduce.hip', 'BESST_SCAN_FREE_MAX_BLOCKS'),
        MSD_MAX_BLOCKS=_knob('sortreduce.hip', 'BESST_MSD_MAX_BLOCKS'),
        SORT_ITEMS=_knob('common.h', 'BESST_SORT_ITEMS'),
        SMALL_ITEMS=_const('sortreduce.hip', r'kMsdMaxBlocks\) run\(std::integral_constant<int, (\d+)>\{\}\);'),
        THREADS=_const('common.h', r'constexpr int kSortThreads = (\d+);'),
        RIDER_MAX_BYTES=_const(os.path.join('..', 'distributed.py'), r'RIDER_MAX_BYTES = (\d+) \* 1024') * 1024)


K = source_knobs()
THREADS = K['THREADS']
SMALL_TILE = THREADS * K['SMALL_ITEMS']          # 1024 tuples
SORT_TILE = THREADS * K['SORT_ITEMS']            # 4096 tuples
SCAN_FREE_CAP = K['SCAN_FREE_MAX_BLOCKS'] * SMALL_TILE       # 65 536: the largest capacity with the scan-free table
SMALL_TILE_CAP = K['MSD_MAX_BLOCKS'] * SORT_TILE             # 4 194 304: the largest capacity with 1024-tuple tiles
FORMS = ('small tile, scan-free table', 'small tile, row-scanned table', 'sort tile, row-scanned table')


def form_of(cap):
    """(form, items per thread) launch_partition picks for a capacity."""
    nb_sort = -(-cap // SORT_TILE)
    if nb_sort <= K['MSD_MAX_BLOCKS']:
        nb = -(-cap // SMALL_TILE)
        return (FORMS[0] if nb <= K['SCAN_FREE_MAX_BLOCKS'] else FORMS[1]), K['SMALL_ITEMS']
    return FORMS[2], K['SORT_ITEMS']


def region_bytes(pair_cap):
    return HEADER_BYTES + pair_cap * 20


def stride_bytes(pair_cap, rider_bytes):
    return (region_bytes(pair_cap) + 7) // 8 * 8 + (rider_bytes + 7) // 8 * 8


# ---- the model ---------------------------------------------------------------------------------------------------------
WRONG_MODELS = collections.OrderedDict([
    # name -> (what is wrong, the design that tells it apart)
    ('rounds_lane_major', ('the rounds of a wave ranked lane-major', 'stability_every_lane')),
    ('waves_reversed', ('the four waves of a tile stitched in the wrong order', 'stability_per_wave')),
    ('n_from_capacity', ('n taken from the capacity', 'sizes_stale_keys_behind_n')),
    ('count_not_clamped', ('the sent count not clamped to pair_capacity', 'overflow_cap_plus_1')),
    ('base_by_sent', ('the global base advanced by the sent count instead of the source\'s total', 'stability_alternate')),
    ('shift_above_drop_plus_one', ('the shift only at idx > drop + 1', 'heads_shift_neighbour')),
    ('no_shift_off_owner', ('no shift on the ranks that do not own the key', 'heads_shift_neighbour')),
    ('prev_from_empty_source', ('previous observations taken from a source without a reaching record', 'heads_junk_in_empty_source')),
    ('second_call_keeps_prev', ('the second call keeping the previous observations', 'heads_double_call_on_duplicate')),
    ('duplicate_dropped_without_detect', ('a duplicate dropped without detect_duplicate', 'heads_matrix_count')),
    ('hash_shift_16', ('the hash shifted by 16', 'worlds_8_ids_below_2_15')),
    ('hash_on_larger_node', ('the hash taken on the larger node', 'worlds_8_ids_below_2_15')),
    ('corrections_in_first_words', ('the corrections added to the rider\'s first eight words', 'rider_257_words_heads')),
])
# `shift at idx >= drop`, which the list of wrong models began with, is NOT one: a tuple whose idx equals the drop is the
# dropped head's own tuple - its owner skips it (or never got it, where the region was cut short), no other rank holds it -
# so `>=` and `>` give the same output in every state the headers can describe (tests/test_exchange_design.py proves that
# over all designs).  The neighbour that CAN be told apart, the shift starting one tuple late, stands in its place.
EQUIVALENT_MODELS = ('shift_ge_drop',)


def owner(scaffold, world, wrong=None):
    """Owner rank of a scaffold's edges: ((id * 2654435761 mod 2^32) >> 15) % world."""
    shift = 16 if wrong == 'hash_shift_16' else 15
    return (((int(scaffold) * HASH) % (1 << 32)) >> shift) % world


def owners_of_keys(keys, node_bits, world, wrong=None):
    """Owner of every key: key = ((min_node << node_bits) | max_node) << 1 | fishy, node = scaffold * 2 + side; the
    owner is taken from the min node's scaffold (32 bits of it)."""
    k = np.asarray(keys, dtype=np.uint64)
    if wrong == 'hash_on_larger_node':
        scaf = ((k >> np.uint64(1)) & np.uint64((1 << node_bits) - 1)) >> np.uint64(1)
    else:
        scaf = (k >> np.uint64(2 + node_bits)) & np.uint64(0xffffffff)
    shift = 16 if wrong == 'hash_shift_16' else 15
    h = (scaf * np.uint64(HASH)) & np.uint64(0xffffffff)
    return ((h >> np.uint64(shift)) % np.uint64(world)).astype(np.int64)


def _rank_order(n, items, wrong):
    """The order in which the tuples of a stream are ranked inside their owner's region: stream order - the wrong models
    rank a wave's rounds lane-major, or stitch a tile's waves from the last to the first."""
    i = np.arange(n, dtype=np.int64)
    if wrong not in ('rounds_lane_major', 'waves_reversed'):
        return i
    per_wave = items * 64
    tile, wave = i // (THREADS * items), (i % (THREADS * items)) // per_wave
    rnd, lane = (i % per_wave) // 64, i % 64
    if wrong == 'rounds_lane_major':
        return np.lexsort((rnd, lane, wave, tile))
    return np.lexsort((lane, rnd, -wave, tile))


Region = collections.namedtuple('Region', 'hdr keys payload idx rider')


def partition(keys, payload, n, cap, node_bits, world, pair_cap, rider=None, slice_info=None, wrong=None):
    """What a source's send buffer holds -> list of `world` Regions.  hdr: {word: value} of the DEFINED header words -
    0 sent, 1 wanted, 2 the source's total, 3 zero; 4..11 the slice description where one is given; 12, 13 (owner,
    position in the owner's region) where the head's tuple is in the stream.  keys / payload / idx: the first
    min(wanted, pair_cap) tuples of the owner, in stream order, idx their stream positions.  rider: the source's rider."""
    n_eff = min(int(n), int(cap))
    if wrong == 'n_from_capacity':
        n_eff = int(cap)
    k = np.asarray(keys[:n_eff], dtype=np.uint64)
    pl = np.asarray(payload[:n_eff], dtype=np.uint64)
    own = owners_of_keys(k, node_bits, world, wrong)
    order = _rank_order(n_eff, form_of(cap)[1], wrong)
    own_ranked = own[order]
    info = None if slice_info is None else [int(x) for x in slice_info]
    head = info[7] if info is not None and 0 <= info[7] < n_eff else None
    head_at = None
    regions = []
    for d in range(world):
        sel = order[own_ranked == d]
        tot = len(sel)
        sent = sel[:min(tot, pair_cap)]
        hdr = {0: tot if wrong == 'count_not_clamped' else len(sent), 1: tot, 2: n_eff, 3: 0}
        if info is not None:
            for j in range(8):
                hdr[4 + j] = info[j] & 0xffffffff
        if head is not None and own[head] == d:
            head_at = (d, int(np.nonzero(sel == head)[0][0]))
        regions.append(Region(hdr, k[sent], pl[sent], sent.astype(np.uint32),
                              None if rider is None else np.asarray(rider, dtype=np.uint64)))
    if head_at is not None:
        for r in regions:
            r.hdr[12], r.hdr[13] = head_at
    return regions


def render(regions, pair_cap, rider_bytes, canary=CANARY):
    """The send buffer byte for byte: the canary wherever `partition` defines nothing."""
    stride = stride_bytes(pair_cap, rider_bytes)
    buf = np.full(len(regions) * stride, canary, dtype=np.uint8)
    for d, r in enumerate(regions):
        base = d * stride
        words = buf[base:base + HEADER_BYTES].view(np.uint32)
        for w, v in r.hdr.items():
            words[w] = v
        c = len(r.keys)
        assert c <= pair_cap
        buf[base + 64:base + 64 + 8 * c].view(np.uint64)[:] = r.keys
        buf[base + 64 + 8 * pair_cap:base + 64 + 8 * pair_cap + 8 * c].view(np.uint64)[:] = r.payload
        buf[base + 64 + 16 * pair_cap:base + 64 + 16 * pair_cap + 4 * c].view(np.uint32)[:] = r.idx
        if rider_bytes:
            off = base + (region_bytes(pair_cap) + 7) // 8 * 8
            buf[off:off + rider_bytes].view(np.uint64)[:] = r.rider
    return buf


CE = collections.namedtuple('CE', 'count too_long dup nus keep')


def create_edge(obs, prev, accept, twice, mapq0, detect, wrong=None):
    """The CreateEdge calls of one record (oracle/py_oracle.py:511-530) -> what they add to count, too_long,
    nr_of_duplicates, non_unique_for_scaf, and whether the record's tuple stays."""
    count = too_long = dup = nus = 0
    keep = False
    for call in range(2 if twice else 1):
        if mapq0:
            nus += 1
        against = prev if (call == 0 or wrong == 'second_call_keeps_prev') else (-1, -1)
        if tuple(obs) == tuple(against):
            dup += 1
            if detect:
                break
            if wrong == 'duplicate_dropped_without_detect':
                continue
        if accept:
            count += 1
            keep = True
        else:
            too_long += 1
    return CE(count, too_long, dup, nus, keep)


def _s32(x):
    x = int(x) & 0xffffffff
    return x - (1 << 32) if x >= 1 << 31 else x


Unpacked = collections.namedtuple('Unpacked', 'keys payload gidx n_out overflow rider_sum corrections all_slice_info')


def unpack(regions, world, pair_cap, rank, speculative, detect, wrong=None):
    """What receiver `rank` makes of the regions its `world` sources sent it (regions[s]: the Region source s addressed
    to this rank) -> keys, payload and gidx in arrival order, n_out, the overflow flag, the rider sums (None without a
    rider) with the counter corrections in their last eight words, the corrections themselves (eight signed words:
    count, non_unique, non_unique_for_scaf, nr_of_duplicates, too_long, fishy, n_tuples, n_reach - what lands in
    `counters` where there is no rider), and all_slice_info (None unless speculative)."""
    assert len(regions) == world
    keys, payload, gidx = [], [], []
    gbase, over = 0, False
    prev = (-1, -1)
    corr = [0] * 8
    all_info = []
    for r in regions:
        cnt, want, tot = r.hdr[0], r.hdr[1], r.hdr[2]
        drop_local = drop_src = -1
        if speculative:
            info = [_s32(r.hdr[4 + j]) for j in range(8)]
            all_info.append(info)
            any_reach, head, flags = info[0] != 0, info[3] != 0, info[6]
            if head:
                d = create_edge((info[4], info[5]), prev, bool(flags & 1), bool(flags & 2), bool(flags & 4), detect, wrong)
                corr[0] += d.count
                corr[2] += d.nus
                corr[3] += d.dup
                corr[4] += d.too_long
                if (flags & 8) and not d.keep:
                    drop_src = info[7]
                    if r.hdr.get(12) == rank and r.hdr.get(13) < cnt:
                        drop_local = r.hdr[13]
                    corr[6] -= 1
            if any_reach or wrong == 'prev_from_empty_source':
                prev = (info[1], info[2])
        m = min(cnt, len(r.keys))
        stay = np.arange(m) != drop_local
        idx = r.idx[:m].astype(np.int64)
        shift = np.zeros(m, bool)
        if drop_src >= 0:
            shift = idx > drop_src
            if wrong == 'shift_above_drop_plus_one':
                shift = idx > drop_src + 1
            if wrong == 'shift_ge_drop':
                shift = idx >= drop_src
            if wrong == 'no_shift_off_owner' and r.hdr.get(12) != rank:
                shift = np.zeros(m, bool)
        keys.append(r.keys[:m][stay])
        payload.append(r.payload[:m][stay])
        gidx.append(((gbase + idx - shift)[stay] & 0xffffffff).astype(np.uint32))
        gbase += (cnt if wrong == 'base_by_sent' else tot) - (1 if drop_src >= 0 else 0)
        over = over or want > cnt
    rider_sum = None
    if regions[0].rider is not None and len(regions[0].rider):
        words = len(regions[0].rider)
        total = [sum(int(r.rider[i]) for r in regions) % (1 << 64) for i in range(words)]
        if speculative:
            first = 0 if wrong == 'corrections_in_first_words' else words - 8
            for j in range(8):
                total[first + j] = (total[first + j] + corr[j]) % (1 << 64)
        rider_sum = np.array(total, dtype=np.uint64)
    keys = np.concatenate(keys).astype(np.uint64)
    return Unpacked(keys, np.concatenate(payload).astype(np.uint64), np.concatenate(gidx).astype(np.uint32),
                    len(keys), over, rider_sum, corr if speculative else [0] * 8,
                    np.array(all_info, dtype=np.int32).reshape(world, 8) if speculative else None)


# ---- building keys ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scaffolds_of_owners(world, lo, hi, per=8):
    """-> tuple over the owners of `world`: the first `per` scaffold ids in [lo, hi) that each owns."""
    pool = [[] for _ in range(world)]
    missing = world
    for s in range(lo, hi):
        p = pool[owner(s, world)]
        if len(p) < per:
            p.append(s)
            if len(p) == per:
                missing -= 1
                if not missing:
                    break
    assert not missing, 'ids %d .. %d do not give every owner of %d its %d scaffolds' % (lo, hi, world, per)
    return tuple(tuple(p) for p in pool)


def make_keys(owners, world, node_bits, lo=1, fishy=None):
    """One key per entry of `owners` (the owner wanted for that tuple): the min node's scaffold taken in turn from the
    scaffolds that owner has at or above `lo`, either side, the max node a little above the min node."""
    owners = np.asarray(owners, dtype=np.int64)
    if node_bits == 1:                                       # nodes 0 and 1 of scaffold 0: one pair, one owner
        assert not owners.any()
        k = np.full(len(owners), 2, dtype=np.uint64)
    else:
        hi = (1 << (node_bits - 1)) - 8
        pool = np.array(scaffolds_of_owners(world, lo, hi), dtype=np.int64)          # world x per
        i = np.arange(len(owners), dtype=np.int64)
        scaf = pool[owners, (i // 3) % pool.shape[1]]
        lo_node = scaf * 2 + i % 2
        hi_node = lo_node + 1 + i % 5
        k = (((lo_node << node_bits) | hi_node) << 1).astype(np.uint64)
    if fishy is not None:
        k = k | np.asarray(fishy, dtype=np.uint64)
    return k


def make_payload(keys, seed):
    """Distinct observations per tuple (a region's order is then visible in the payload too), the graph mask a function
    of the key: the payload format of stage 2 (tests/sort_design.make_payload)."""
    from tests import sort_design as SD
    return SD.make_payload(np.asarray(keys, dtype=np.uint64), np.random.default_rng(seed))


# ---- designs ---------------------------------------------------------------------------------------------------------------
# One source of an exchange.  n_reported: what *n_tuples holds (may exceed the capacity); keys / payload: `cap` slots, the
# ones behind n included; rider: uint64 words or None; slice_info: 8 int32 or None.
Source = collections.namedtuple('Source', 'keys payload n_reported cap rider slice_info')
# claims: [(text, predicate over the census)]; ranks: the receivers checked (None: all); round_trip: the exchange is
# untruncated and free of heads, so partition -> unpack -> reduce must give the whole stream's edge table
Exchange = collections.namedtuple('Exchange', 'name world pair_cap node_bits sources speculative detect ranks claims '
                                              'round_trip null_all_info')


def _source(owners, world, node_bits, cap=None, n_reported=None, seed=0, lo=1, fishy=None, stale_owner=None, rider=None,
            slice_info=None):
    n = len(owners)
    cap = n if cap is None else cap
    k = make_keys(owners, world, node_bits, lo, fishy)
    keys = np.zeros(max(cap, 1), dtype=np.uint64)
    payload = np.zeros(max(cap, 1), dtype=np.uint64)
    m = min(n, cap)
    keys[:m] = k[:m]
    payload[:m] = make_payload(k[:m], seed + n)
    if stale_owner is not None and cap > n:
        stale = make_keys(np.full(cap - n, stale_owner), world, node_bits, lo)
        keys[n:cap] = stale
        payload[n:cap] = make_payload(stale, seed + 1)
    return Source(keys, payload, n if n_reported is None else n_reported, cap, rider, slice_info)


def _tiny(s, world, node_bits, n=None, rider=None, slice_info=None, lo=1):
    """The small stream the sources of an exchange hold where the design is about another source."""
    n = (5 + 3 * s) % 23 if n is None else n
    owners = (np.arange(n) * 5 + s) % world
    return _source(owners, world, node_bits, cap=max(n, 1), seed=1000 + s, rider=rider, slice_info=slice_info, lo=lo)


def _pair_cap_for(sources, world, node_bits):
    most = 0
    for s in sources:
        n = min(s.n_reported, s.cap)
        if n:
            most = max(most, int(np.bincount(owners_of_keys(s.keys[:n], node_bits, world), minlength=world).max()))
    return most + 2 + (most & 1)


def _exchange(name, world, node_bits, first, claims, pair_cap=None, speculative=False, detect=True, ranks=None,
              round_trip=True, others=None, null_all_info=False):
    """An exchange whose source 0 is `first`; the others hold tiny streams unless given."""
    sources = [first] + (list(others) if others is not None else
                         [_tiny(s, world, node_bits, rider=first.rider) for s in range(1, world)])
    assert len(sources) == world
    pc = pair_cap or _pair_cap_for(sources, world, node_bits)
    return Exchange(name, world, pc, node_bits, sources, speculative, detect, ranks, claims, round_trip, null_all_info)


# ---- the census --------------------------------------------------------------------------------------------------------------
Census = collections.namedtuple('Census', 'n form tile owners changes totals truncated canary_bytes infos ex')


def census(ex, s=0):
    """Facts about source s of an exchange, from its inputs alone: the tuples the kernels will see (n), the form and tile
    its capacity picks, the owner of every tuple, the stream positions where the owner changes, every region's total, the
    truncated regions, and how many bytes of the send buffer must keep the canary."""
    src = ex.sources[s]
    n = min(src.n_reported, src.cap)
    form, items = form_of(src.cap)
    own = owners_of_keys(src.keys[:n], ex.node_bits, ex.world)
    changes = np.nonzero(np.diff(own))[0] + 1
    totals = np.bincount(own, minlength=ex.world)
    rider_bytes = 0 if src.rider is None else 8 * len(src.rider)
    defined = 0
    head_in = src.slice_info is not None and 0 <= int(src.slice_info[7]) < n
    for t in totals:
        defined += 16 + (32 if src.slice_info is not None else 0) + (8 if head_in else 0) + 20 * min(int(t), ex.pair_cap) + rider_bytes
    canary = ex.world * stride_bytes(ex.pair_cap, rider_bytes) - defined
    infos = [None if x.slice_info is None else [int(v) for v in x.slice_info] for x in ex.sources]
    return Census(n, form, THREADS * items, own, changes, totals, [d for d in range(ex.world) if totals[d] > ex.pair_cap], canary,
                  infos, ex)


def head_place(c, s):
    """Where the head tuple of source s goes: (owner, position in the owner's region, tuples sent to that owner)."""
    cs = census(c.ex, s)
    pos = c.infos[s][7]
    who = int(cs.owners[pos])
    return who, int((cs.owners[:pos] == who).sum()), min(int(cs.totals[who]), c.ex.pair_cap)


def _only_at(c, who, at):
    return list(np.nonzero(c.owners == who)[0]) == list(at)


# -- forms
def form_designs():
    out = []
    caps = [SMALL_TILE, SCAN_FREE_CAP, SCAN_FREE_CAP + 1, SMALL_TILE_CAP, SMALL_TILE_CAP + 1]
    want = [FORMS[0], FORMS[0], FORMS[1], FORMS[1], FORMS[2]]
    for cap, form in zip(caps, want):
        owners = np.arange(70) % 2
        out.append(_exchange('forms_cap_%d_few' % cap, 2, 16, _source(owners, 2, 16, cap=cap, stale_owner=1 if cap <= SCAN_FREE_CAP + 1 else None, seed=cap),
                             [('capacity %d takes the form: %s' % (cap, form), lambda c, f=form: c.form == f),
                              ('70 tuples, the owner changing at every lane', lambda c: c.n == 70 and len(c.changes) == 69)]))
    for cap, form in zip(caps[1:3], want[1:3]):
        owners = (np.arange(cap) // 7 + np.arange(cap) // 1000) % 3
        out.append(_exchange('forms_cap_%d_full' % cap, 3, 16, _source(owners, 3, 16, cap=cap, seed=cap + 1),
                             [('full: n == capacity == %d, form: %s' % (cap, form), lambda c, f=form, n=cap: c.form == f and c.n == n),
                              ('more than one tile for every owner', lambda c: int(c.totals.min()) > c.tile)]))
    return out


# -- sizes
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def size_designs():
    out = []
    for n in SIZES:
        out.append(_exchange('sizes_n_%d' % n, 3, 16, _source(np.arange(n) % 3, 3, 16, cap=2048, stale_owner=2, seed=n),
                             [('n = %d in 2048 slots' % n, lambda c, n=n: c.n == n)]))
    for cap in (SMALL_TILE, SMALL_TILE + 1):
        out.append(_exchange('sizes_n_equals_capacity_%d' % cap, 3, 16, _source((np.arange(cap) // 5) % 3, 3, 16, cap=cap, seed=cap),
                             [('n == capacity == %d, %s a tile border' % (cap, 'on' if cap % SMALL_TILE == 0 else 'one behind'),
                               lambda c, cap=cap: c.n == cap and len(c.ex.sources[0].keys) == cap)]))
    cap = 1029
    src = _source(np.arange(cap) % 3, 3, 16, cap=cap, n_reported=cap + 5, seed=7)
    out.append(_exchange('sizes_n_reported_beyond_capacity', 3, 16, src,
                         [('*n_tuples = capacity + 5 is clamped to the capacity', lambda c: c.n == 1029)]))
    src = _source(np.arange(1000) % 2, 3, 16, cap=2048, stale_owner=2, seed=8)
    out.append(_exchange('sizes_stale_keys_behind_n', 3, 16, src,
                         [('owner 2 has no tuple in front of n', lambda c: c.totals[2] == 0 and c.n == 1000),
                          ('every slot behind n holds a key of owner 2', lambda c, s=src: bool(
                              (owners_of_keys(s.keys[1000:], 16, 3) == 2).all()) and len(s.keys) == 2048)]))
    return out


# -- stability
def stability_designs():
    out = []
    n = 2 * SMALL_TILE + 300
    i = np.arange(n)
    out.append(_exchange('stability_every_lane', 3, 16, _source(i % 3, 3, 16, seed=1),
                         [('the owner changes at every lane', lambda c: len(c.changes) == c.n - 1)]))
    for name, unit in (('round', 64), ('wave', 64 * K['SMALL_ITEMS']), ('tile', SMALL_TILE)):
        m = n if unit < SMALL_TILE else 3 * SMALL_TILE + 300
        out.append(_exchange('stability_per_%s' % name, 3, 16, _source((np.arange(m) // unit) % 3, 3, 16, seed=unit),
                             [('the owner is constant per %s and changes on every %s border' % (name, name),
                               lambda c, u=unit: list(c.changes) == list(range(u, c.n, u)))]))
    own = i % 2
    last_wave, last_tile = 64 * K['SMALL_ITEMS'] - 1, SMALL_TILE - 1
    own[[last_wave, last_tile, n - 1]] = 2
    out.append(_exchange('stability_last_of_wave_tile_stream', 3, 16, _source(own, 3, 16, seed=2),
                         [('owner 2 only as the last tuple of a wave, of a tile and of the stream',
                           lambda c, at=(last_wave, last_tile, n - 1): _only_at(c, 2, at))]))
    out.append(_exchange('stability_alternate', 3, 16, _source(i % 2, 3, 16, seed=3),
                         [('two owners alternate: each idx column is an arithmetic progression',
                           lambda c: bool((np.diff(np.nonzero(c.owners == 0)[0]) == 2).all() and (np.diff(np.nonzero(c.owners == 1)[0]) == 2).all())),
                          ('owner 2 is left with an empty region', lambda c: c.totals[2] == 0)]))
    out.append(_exchange('stability_one_owner', 3, 16, _source(np.full(n, 1), 3, 16, seed=4),
                         [('all tuples go to owner 1', lambda c: list(c.totals) == [0, c.n, 0])]))
    out.append(_exchange('stability_one_each', 8, 16, _source(np.arange(8)[::-1].copy(), 8, 16, seed=5),
                         [('exactly one tuple per owner', lambda c: list(c.totals) == [1] * 8)]))
    return out


def scaffold_ids(c):
    """The min node's scaffold id of every tuple of every source."""
    ids = [s.keys[:min(s.n_reported, s.cap)] >> np.uint64(2 + c.ex.node_bits) for s in c.ex.sources]
    return np.concatenate(ids).astype(np.int64)


def _id_range_holds(c, name, nb):
    ids = scaffold_ids(c)
    keys = np.concatenate([s.keys[:min(s.n_reported, s.cap)] for s in c.ex.sources])
    if int(keys.max()).bit_length() > 2 * nb + 1:
        return False
    if name == 'below_2_15':                                 # the hash's shift leaves small products
        return 1 <= int(ids.min()) and int(ids.max()) < 1 << 15
    if name == 'around_2_17':                                # ids on both sides of 2^17
        return int(ids.min()) < 1 << 17 <= int(ids.max()) and int(ids.max()) < (1 << 17) + 4096
    return int(ids.min()) > 1 << 27 and nb == 29 and int(keys.max()).bit_length() >= 58      # 59-bit keys but for the top bit


# -- worlds
def world_designs():
    out = []
    for world in (1, 2, 3, 8, 64, 255, 256):
        n = SMALL_TILE + 476                                 # 1500: the last tile is ragged
        own = (np.arange(n) * 7) % world
        if world > 1:
            own[-69::2] = world - 1                          # the last owner sits next to the lanes behind n
        ranks = None if world <= 64 else sorted({0, 1, world // 2, world - 2, world - 1})
        out.append(_exchange('worlds_%d' % world, world, 16, _source(own, world, 16, seed=world), [
            ('world %d, every owner present' % world, lambda c, w=world: len(c.totals) == w and int(c.totals.min()) >= 1),
            ('the last tile is ragged and ends on tuples of the last owner',
             lambda c, w=world: c.n % c.tile != 0 and c.owners[-1] == w - 1)], ranks=ranks))
    for name, nb, lo in (('below_2_15', 16, 1), ('around_2_17', 19, (1 << 17) - 40), ('above_2_27', 29, (1 << 27) + 1)):
        src = _source(np.arange(700) % 8, 8, nb, seed=nb, lo=lo)
        out.append(_exchange('worlds_8_ids_%s' % name, 8, nb, src, [
            ('scaffold ids %s, node_bits %d' % (name.replace('_', ' ').replace('2 ', '2^'), nb),
             lambda c, name=name, nb=nb: _id_range_holds(c, name, nb))],
            others=[_tiny(s, 8, nb, lo=lo) for s in range(1, 8)]))
    src = _source(np.zeros(300, np.int64), 3, 1, seed=9, fishy=np.arange(300) % 2)
    out.append(_exchange('worlds_node_bits_1', 3, 1, src, [
        ('node_bits 1: one node pair, the fishy bit set and clear on it',
         lambda c, s=src: sorted(set(s.keys[:300].tolist())) == [2, 3])],
        others=[_source(np.zeros(4, np.int64), 3, 1, seed=10 + s) for s in (1, 2)], round_trip=False))
    src = _source(np.arange(400) // 2 % 3, 3, 16, seed=11)
    k = src.keys.copy()
    k[:400] = (k[:400] & ~np.uint64(1))
    k[1:400:2] = k[0:399:2] | np.uint64(1)                   # each odd tuple: the tuple before it with the fishy bit set
    src = src._replace(keys=k)
    out.append(_exchange('worlds_fishy_pair', 3, 16, src, [
        ('the fishy bit set and clear on one node pair, next to each other',
         lambda c, s=src: bool(((s.keys[1:400:2] ^ s.keys[0:399:2]) == 1).all()))], round_trip=False))
    return out


# -- overflow
def overflow_designs():
    out = []
    tile_cap = SMALL_TILE + 2                                # the smallest even value above a tile
    for pc in (2, 64, tile_cap):
        for name, tot in (('cap_minus_1', pc - 1), ('cap', pc), ('cap_plus_1', pc + 1), ('twice_cap', 2 * pc)):
            if pc != 64 and name == 'twice_cap':
                continue
            own = [1] * tot                                  # owner 1's tuples, two of owner 0 and one of owner 2 among them
            own.insert(1, 0)
            own.insert(len(own) // 2, 0)
            own.insert(len(own) - 1, 2)
            own = np.array(own)
            label = 'overflow_%s' % name if pc == 64 else 'overflow_pair_cap_%d_%s' % (pc, name)
            trunc = [1] if tot > pc else []
            out.append(_exchange(label, 3, 16, _source(own, 3, 16, seed=pc + tot), [
                ('owner 1 is sent %d tuples with pair_capacity %d' % (tot, pc), lambda c, t=tot: c.totals[1] == t),
                ('truncated regions: %s' % trunc, lambda c, t=trunc: c.truncated == t),
                ('canary bytes left in the send buffer', lambda c: c.canary_bytes > 0)],
                pair_cap=pc, round_trip=not trunc,
                others=[_tiny(s, 3, 16, n=min(pc - 1, 5)) for s in (1, 2)]))
    return out


# -- riders
NEAR_2_63 = (1 << 62) - 3


def _rider(words, seed, top=None):
    r = (np.arange(words, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)) >> np.uint64(8)
    if top is not None and words:
        r[::5] = np.uint64(top)
    return r


def _rider_sums_carry(c):
    """The exact sums of the sources' rider words: some sum has bit 63 set although no addend has, none reaches 2^64."""
    words = [[int(x) for x in s.rider] for s in c.ex.sources]
    sums = [sum(col) for col in zip(*words)]
    return all(x < 1 << 63 for w in words for x in w) and any(x >> 63 for x in sums) and all(x < 1 << 64 for x in sums)


def rider_designs():
    out = []
    for words in (0, 1, 8, THREADS, THREADS + 1, K['RIDER_MAX_BYTES'] // 8):
        rid = None if not words else _rider(words, 1, NEAR_2_63)
        others = [_tiny(s, 2, 16, rider=None if not words else _rider(words, 1 + s, NEAR_2_63 + 9)) for s in (1,)]
        out.append(_exchange('rider_%d_words' % words, 2, 16, _source(np.arange(300) % 2, 2, 16, seed=words, rider=rid), [
            ('a rider of %d bytes' % (8 * words), lambda c, w=words: (c.ex.sources[0].rider is None and not w) or len(c.ex.sources[0].rider) == w),
            ('two sources\' words near 2^62: the sum carries into bit 63 and not out of it',
             lambda c, w=words: not w or _rider_sums_carry(c))],
            others=others))
    return out


# -- heads: synthetic slice descriptions
def _info(any_reach=0, tail=(0, 0), head=0, obs=(0, 0), flags=0, pos=-1):
    return np.array([any_reach, tail[0], tail[1], head, obs[0], obs[1], flags, pos], dtype=np.int32)


def _head_source(s, world, info, n=7, rider=None, owners=None):
    owners = (np.arange(n) * 3 + s) % world if owners is None else owners
    return _source(owners, world, 16, cap=max(len(owners), 1), seed=2000 + s, slice_info=info, rider=rider)


RELATIONS = ('equal', 'different', 'minus_one')


def head_relations(c):
    """Per source with a head, from the slice descriptions alone: (flag word, how the head's observations stand to the
    previous observations that reach it - the tail of the nearest earlier source with a reaching record, (-1, -1) for the
    first) -> list in source order; 'initial' where nothing precedes."""
    out, prev = [], None
    for info in c.infos:
        if info[3]:
            obs = info[4:6]
            if obs == [-1, -1] and prev != [-1, -1] and prev is not None:
                rel = 'minus_one'
            elif prev is None:
                rel = 'initial'
            else:
                rel = 'equal' if obs == prev else 'different'
            out.append((info[6], rel))
        if info[0]:
            prev = info[1:3]
    return out


def heads_matrix(detect, rider_words=0):
    """Source 0 opens the chain (its head meets the initial (-1, -1): once equal to it, see heads_first_source); sources
    1 .. 48 hold every flag combination against a head equal to the incoming previous observations, different from
    them, and equal to (-1, -1).  A head whose flags say `tuple emitted` names tuple 2 of its stream."""
    world = 1 + 16 * len(RELATIONS)
    tails = [(100 + s, 200 + s) for s in range(world)]
    sources = []
    combos = [None]
    for s in range(world):
        rid = _rider(rider_words, s) if rider_words else None
        if s == 0:
            sources.append(_head_source(0, world, _info(1, tails[0], 1, (50, 60), 1 | 8, 2), rider=rid))
            continue
        flags, rel = (s - 1) % 16, RELATIONS[(s - 1) // 16]
        obs = tails[s - 1] if rel == 'equal' else ((300 + s, 400 + s) if rel == 'different' else (-1, -1))
        combos.append((flags, rel))
        sources.append(_head_source(s, world, _info(1, tails[s], 1, obs, flags, 2 if flags & 8 else -1), rider=rid))
    name = 'heads_matrix_%s' % ('detect' if detect else 'count') + ('_rider' if rider_words else '')
    claims = [('flags 0..15 x head equal / different / (-1, -1), detect_duplicate %s' % detect,
               lambda c: sorted(head_relations(c)[1:]) == sorted((f, r) for f in range(16) for r in RELATIONS) and
               all(head_place(c, s)[2] > head_place(c, s)[1] for s in range(len(c.infos)) if c.infos[s][6] & 8) and
               all((c.infos[s][7] >= 0) == bool(c.infos[s][6] & 8) for s in range(len(c.infos))))]
    return Exchange(name, world, 8, 16, sources, True, detect, None, claims, False, False), combos


def head_designs():
    out = [heads_matrix(True)[0], heads_matrix(False)[0]]
    W = 4
    # the first source's head meets the initial (-1, -1)
    src = [_head_source(0, W, _info(1, (5, 6), 1, (-1, -1), 2, -1)),
           _head_source(1, W, _info(1, (7, 8), 1, (5, 6), 1 | 8, 0)),
           _head_source(2, W, _info(0)), _head_source(3, W, _info(0), n=0)]
    out.append(Exchange('heads_first_source', W, 8, 16, src, True, True, None, [
        ('source 0\'s head observes (-1, -1); source 1\'s head duplicates source 0\'s tail, its tuple is tuple 0',
         lambda c: c.infos[0][4:6] == [-1, -1] and c.infos[1][4:6] == c.infos[0][1:3] and c.infos[1][7] == 0 and
         not c.infos[2][0] and census(c.ex, 3).n == 0)], False, False))
    # a head that duplicates the tail before it, under the double call, duplicates counted and kept
    src = [_head_source(0, 2, _info(1, (5, 6), 0)), _head_source(1, 2, _info(1, (7, 8), 1, (5, 6), 1 | 2 | 8, 1))]
    out.append(Exchange('heads_double_call_on_duplicate', 2, 8, 16, src, True, False, None, [
        ('the head repeats the tail before it, flags accept | double call | emitted, detect_duplicate off',
         lambda c: c.infos[1][4:6] == c.infos[0][1:3] and c.infos[1][6] == 11 and not c.ex.detect)], False, False))
    # the chain through one and through three sources without a reaching record
    for gap in (1, 3):
        world = gap + 2
        src = [_head_source(0, world, _info(1, (31, 32), 1, (9, 9), 1 | 8, 1))]
        src += [_head_source(1 + g, world, _info(0), n=3 * g) for g in range(gap)]
        src.append(_head_source(world - 1, world, _info(1, (41, 42), 1, (31, 32), 1 | 2 | 8, 3)))
        out.append(Exchange('heads_chain_through_%d' % gap, world, 8, 16, src, True, True, None, [
            ('%d sources with any = 0 between a tail and the head that duplicates it' % gap,
             lambda c, g=gap: not any(c.infos[1 + j][0] for j in range(g)) and c.infos[g + 1][4:6] == c.infos[0][1:3] and
             len(c.infos) == g + 2)], False, False))
    src = [_head_source(0, 3, _info(1, (31, 32), 1, (9, 9), 1 | 8, 1)),
           _head_source(1, 3, _info(0, (77, 78), 0, (0, 0), 0, -1)),
           _head_source(2, 3, _info(1, (41, 42), 1, (77, 78), 1 | 8, 3))]
    out.append(Exchange('heads_junk_in_empty_source', 3, 8, 16, src, True, True, None, [
        ('source 1 has any = 0 and junk in words 5 and 6 that source 2\'s head repeats',
         lambda c: not c.infos[1][0] and c.infos[1][1:3] == c.infos[2][4:6] != [0, 0] and c.infos[0][1:3] != c.infos[2][4:6])], False, False))
    # three dropped heads: on different owners, and on one owner
    for same in (False, True):
        world = 4
        src = [_head_source(0, world, _info(1, (11, 12), 0))]
        for s in (1, 2, 3):
            owners = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0])
            pos = 4 if same else 3 + s                       # tuple 4 is owner 0's; tuples 4, 5, 6: owners 0, 1, 2
            src.append(_head_source(s, world, _info(1, (11, 12), 1, (11, 12), 1 | 8, pos), owners=owners))
        out.append(Exchange('heads_three_drops_%s' % ('one_owner' if same else 'three_owners'), world, 8, 16, src, True, True,
                            None, [('three sources whose heads are dropped, %s' % ('all at owner 0' if same else 'at owners 0, 1, 2'),
                                    lambda c, o=[0, 0, 0] if same else [0, 1, 2]: [head_place(c, s)[0] for s in (1, 2, 3)] == o and
                                    all(c.infos[s][4:6] == c.infos[s - 1][1:3] and c.infos[s][6] & 8 for s in (1, 2, 3)))], False, False))
    # the drop first, last, and beyond cnt in a truncated region
    owners = np.array([1, 1, 1, 1, 1, 1, 0, 2])
    for name, pos, pc in (('first', 0, 8), ('last', 5, 6), ('beyond_cnt', 5, 4), ('at_cnt', 4, 4)):
        src = [_head_source(0, 3, _info(1, (21, 22), 0)),
               _head_source(1, 3, _info(1, (23, 24), 1, (21, 22), 1 | 8, pos), owners=owners),
               _head_source(2, 3, _info(1, (25, 26), 1, (90, 91), 1 | 8, 0), n=5)]
        out.append(Exchange('heads_drop_%s' % name, 3, pc, 16, src, True, True, None, [
            ('owner 1 is sent 6 tuples of source 1, pair_capacity %d, the dropped head is its tuple %d' % (pc, pos),
             lambda c, pos=pos, pc=pc: head_place(c, 1) == (1, pos, min(6, pc)) and c.infos[1][4:6] == c.infos[0][1:3])], False, False))
    # a tuple whose idx is the dropped head's idx + 1: on the owner and on a rank that owns neither
    owners = np.array([0, 0, 1, 1, 2, 0, 1])                 # head: tuple 2 (owner 1); tuple 3 owner 1, tuple 4 owner 2
    src = [_head_source(0, 3, _info(1, (21, 22), 0)),
           _head_source(1, 3, _info(1, (23, 24), 1, (21, 22), 1 | 8, 2), owners=owners),
           _head_source(2, 3, _info(0), n=4)]
    out.append(Exchange('heads_shift_neighbour', 3, 8, 16, src, True, True, None, [
        ('the tuple behind the dropped head belongs to the owner, the one after to a bystander',
         lambda c: [int(x) for x in census(c.ex, 1).owners[2:5]] == [1, 1, 2] and c.infos[1][7] == 2 and
         c.infos[1][4:6] == c.infos[0][1:3])],
        False, False))
    out.append(Exchange('heads_null_all_slice_info', 3, 8, 16, src, True, True, None, [
        ('all_slice_info is null', lambda c: c.ex.null_all_info)], False, True))
    # riders under speculative heads: the corrections land in the last eight words
    for words in (8, THREADS + 1):
        ex, _ = heads_matrix(True, rider_words=words)
        out.append(ex._replace(name='rider_%d_words_heads' % words))
    return out


ERROR_CASES = [
    # name, stage, arguments that differ from a valid call
    ('world 0', 'partition', dict(world=0)), ('world 257', 'partition', dict(world=257)),
    ('world 0', 'unpack', dict(world=0)), ('world 257', 'unpack', dict(world=257)),
    ('odd pair_capacity', 'partition', dict(pair_cap=7)), ('zero pair_capacity', 'partition', dict(pair_cap=0)),
    ('zero pair_capacity', 'unpack', dict(pair_cap=0)),
    ('rider of 12 bytes', 'partition', dict(rider_bytes=12)), ('rider of 12 bytes', 'unpack', dict(rider_bytes=12)),
    ('rider of 8 bytes with speculative heads', 'unpack', dict(rider_bytes=8, speculative=1)),
    ('rank outside the world with speculative heads', 'unpack', dict(rank=3, speculative=1)),
    ('negative rank with speculative heads', 'unpack', dict(rank=-1, speculative=1)),
]


_CACHE = collections.OrderedDict()


def all_designs():
    """name -> Exchange, built once per process."""
    if not _CACHE:
        for ex in (form_designs() + size_designs() + stability_designs() + world_designs() + overflow_designs() +
                   rider_designs() + head_designs()):
            assert ex.name not in _CACHE, ex.name
            _CACHE[ex.name] = ex
    return _CACHE


def rider_bytes_of(ex):
    r = ex.sources[0].rider
    return 0 if r is None else 8 * len(r)


def model_partitions(ex, wrong=None):
    """[source][destination] -> Region."""
    return [partition(s.keys, s.payload, s.n_reported, s.cap, ex.node_bits, ex.world, ex.pair_cap, s.rider, s.slice_info, wrong)
            for s in ex.sources]


def model_unpack(ex, rank, parts=None, wrong=None):
    parts = model_partitions(ex, wrong) if parts is None else parts
    return unpack([parts[s][rank] for s in range(ex.world)], ex.world, ex.pair_cap, rank, ex.speculative, ex.detect, wrong)


def ranks_of(ex):
    return list(range(ex.world)) if ex.ranks is None else ex.ranks


def whole_stream(ex):
    """The sources' tuples in global order (keys, payload)."""
    ks = [s.keys[:min(s.n_reported, s.cap)] for s in ex.sources]
    ps = [s.payload[:min(s.n_reported, s.cap)] for s in ex.sources]
    return np.concatenate(ks), np.concatenate(ps)
