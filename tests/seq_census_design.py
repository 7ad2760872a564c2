"""Designed byte streams with their segment tables for the sequence census, scaled by the tile size ``T`` of the kernel
under test (tiles begin at multiples of ``T`` of a stream that lies at an aligned address).  Every builder returns a dict:
``stream`` (bytes), ``seq_off`` / ``seq_len`` (lists, ascending and disjoint, stream positions from 0) and ``borders``, the
names of the borders the design was built to contain - ``has_border`` looks each of them up in the bytes and the table, so
that a builder that drifts away from its purpose fails a test instead of silently testing less."""
import random

from tests import seq_census_model as M

ALPHABET = b'ACGTACGTACGTacgtRYKMBVHDSWrykmbvhdswXx*-.'
LENGTHS = lambda T: [0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T, 3 * T + 5]


def _bases(rng, n):
    """``n`` bytes without N"""
    return bytes(rng.choice(ALPHABET) for _ in range(n))


def _with_runs(rng, n, n_runs=3):
    """``n`` bytes with a few short runs of N / n inside"""
    data = bytearray(_bases(rng, n))
    for _ in range(n_runs if n > 8 else 0):
        at, size = rng.randrange(1, n - 1), rng.choice([1, 2, 3, 17, 40])
        for p in range(at, min(n - 1, at + size)):
            data[p] = rng.choice(b'NNNn')
    return bytes(data)


def lengths_and_alignments(T, seed=1):
    """Rows of every length of LENGTHS, the starts at every alignment 0..15 (twice over: 32 rows), bytes between the rows
    that belong to none."""
    rng = random.Random(seed)
    stream, off, length = bytearray(), [], []
    sizes = LENGTHS(T)
    for k in range(32):
        want = k % 16
        pad = (want - len(stream)) % 16
        stream += _with_runs(rng, pad + (16 if k % 3 == 0 else 0), 1)      # (a spacer, sometimes with N next to the row)
        n = sizes[k % len(sizes)]
        off.append(len(stream))
        length.append(n)
        stream += _with_runs(rng, n)
    stream += _bases(rng, 7)
    return dict(name='lengths_and_alignments', stream=bytes(stream), seq_off=off, seq_len=length,
                borders=['every_length', 'every_alignment', 'row_outside_any_small_window'])


def runs_at_tile_borders(T, seed=2):
    """One row that is the whole stream of 8 T bytes, with runs of N that end on a tile's last byte, start on a tile's
    first, span exactly one tile and span three tiles."""
    rng = random.Random(seed)
    data = bytearray(_bases(rng, 8 * T))
    for lo, hi in ((T - 7, T), (2 * T, 2 * T + 5), (3 * T, 4 * T), (5 * T - 3, 7 * T + 3), (7 * T + 100, 7 * T + 101)):
        for p in range(lo, hi):
            data[p] = ord('N') if p % 5 else ord('n')
    return dict(name='runs_at_tile_borders', stream=bytes(data), seq_off=[0], seq_len=[len(data)],
                borders=['run_ends_on_tile_last_byte', 'run_starts_on_tile_first_byte', 'run_is_one_whole_tile',
                         'run_spans_three_tiles', 'row_is_whole_stream'])


def all_n_and_neighbours(T, seed=3):
    """An all-N row of 3 T + 5 bytes, and rows that end in N directly followed by rows that begin with N: the runs must
    not join across rows."""
    rng = random.Random(seed)
    rows = [b'N' * (3 * T + 5), b'NNNN' + _bases(rng, 50) + b'nnN', b'N' + _bases(rng, T + 3) + b'NN', b'n' * 20,
            _bases(rng, 9) + b'N', b'N']
    off, at = [], 0
    for r in rows:
        off.append(at)
        at += len(r)
    return dict(name='all_n_and_neighbours', stream=b''.join(rows), seq_off=off, seq_len=[len(r) for r in rows],
                borders=['all_n_row_of_3T_plus_5', 'n_suffix_meets_n_prefix'])


def many_short_rows(T, seed=4):
    """300 rows of 0 - 3 bytes inside one tile - more than a wave's lanes - with rows of length 0 in the middle, at the end
    and at the very end of the stream."""
    rng = random.Random(seed)
    stream, off, length = bytearray(_bases(rng, 5)), [], []
    for k in range(300):
        n = (k * 7 + k // 5) % 4
        off.append(len(stream))
        length.append(n)
        stream += bytes(rng.choice(b'ACGTNNnacgtR*') for _ in range(n))
        if k % 11 == 0:
            stream += b'N'                                       # between rows: belongs to none
    off += [len(stream)] * 3                                     # off == the end of the stream
    length += [0] * 3
    assert len(stream) < T
    return dict(name='many_short_rows', stream=bytes(stream), seq_off=off, seq_len=length,
                borders=['300_short_rows_in_one_tile', 'zero_length_rows_middle_and_end', 'zero_length_row_at_stream_end'])


def all_byte_values(T=None, seed=5):
    """Every byte value, in rows of 100 bytes at odd alignments, and once more in one long row."""
    data = bytes(range(256)) + bytes(reversed(range(256))) + bytes(range(256))
    off = [3, 103, 203, 303, 512]
    length = [100, 100, 100, 100, 256]
    return dict(name='all_byte_values', stream=data, seq_off=off, seq_len=length, borders=['all_256_byte_values'])


def all_designs(T):
    return [lengths_and_alignments(T), runs_at_tile_borders(T), all_n_and_neighbours(T), many_short_rows(T),
            all_byte_values(T)]


def has_border(design, border, T):
    stream, off, length = design['stream'], design['seq_off'], design['seq_len']
    rows = list(zip(off, length))
    runs = M.n_runs(stream)
    if border == 'every_length':
        return set(LENGTHS(T)) <= set(length)
    if border == 'every_alignment':
        return {o % 16 for o in off} == set(range(16))
    if border == 'row_outside_any_small_window':
        return len(stream) > 4 * T and len(rows) > 2
    if border == 'run_ends_on_tile_last_byte':
        return any((s + n) % T == 0 and s % T != 0 and n < T for s, n in runs)
    if border == 'run_starts_on_tile_first_byte':
        return any(s % T == 0 and s > 0 and n < T for s, n in runs)
    if border == 'run_is_one_whole_tile':
        return any(s % T == 0 and n == T for s, n in runs)
    if border == 'run_spans_three_tiles':
        return any((s + n - 1) // T - s // T >= 2 and s % T != 0 for s, n in runs)
    if border == 'row_is_whole_stream':
        return rows == [(0, len(stream))]
    if border == 'all_n_row_of_3T_plus_5':
        return any(n == 3 * T + 5 and M.partial(stream[o:o + n])[M.PRE] == n for o, n in rows)
    if border == 'n_suffix_meets_n_prefix':
        return any(n1 > 0 and n2 > 0 and o1 + n1 == o2 and M.CLASS[stream[o2 - 1]] == M.N and M.CLASS[stream[o2]] == M.N
                   for (o1, n1), (o2, n2) in zip(rows[:-1], rows[1:]))
    if border == '300_short_rows_in_one_tile':
        short = [(o, n) for o, n in rows if n <= 3 and o + n <= T]
        return len(short) >= 300 and {n for _, n in short} == {0, 1, 2, 3}
    if border == 'zero_length_rows_middle_and_end':
        return any(n == 0 for n in length[1:-4]) and length[-1] == 0
    if border == 'zero_length_row_at_stream_end':
        return rows[-1] == (len(stream), 0)
    if border == 'all_256_byte_values':
        return any(set(stream[o:o + n]) == set(range(256)) for o, n in rows)
    raise KeyError(border)


def shifted(design, origin):
    """the same table for a stream that begins at stream position ``origin``"""
    return [o + origin for o in design['seq_off']], list(design['seq_len'])
