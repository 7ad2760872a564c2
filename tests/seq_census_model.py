"""The tests' own sequence census: plain Python, written without a look at besst_amd/csrc/seq_census_core.h.

A census is a list of 16 ints (include/besst_amd.h, BESST_CENSUS_*).  ``partial`` counts one byte string the way the device
leaves it (the runs of 'N' at either end open), ``merge`` joins neighbours, ``finalise`` closes the ends; ``whole`` is the
finalised census straight from ``itertools.groupby``, which the other three must add up to.  ``windowed`` walks a stream in
windows as the device protocol does.  ``nx`` / ``lx`` take a list of lengths."""
import itertools

WORDS = 16
LEN, A, C, G, T, N, IUPAC, OTHER, LOWER, PRE, SUF, RUNS, GAPS, GAP_BASES, LONGEST = range(15)

# the class of every byte value, written out: word index of the count it belongs to
CLASS = [OTHER] * 256
for _c, _w in (('A', A), ('C', C), ('G', G), ('T', T), ('N', N)):
    CLASS[ord(_c)] = CLASS[ord(_c.lower())] = _w
for _c in 'YRKMBVHDSW':
    CLASS[ord(_c)] = CLASS[ord(_c.lower())] = IUPAC
CLASS[ord('X')] = IUPAC                                     # upper case only: 'x' has no complement


def n_runs(data):
    """[(start, length)] of the runs of N / n in ``data``"""
    runs, at = [], 0
    for is_n, group in itertools.groupby(bytes(data), key=lambda b: CLASS[b] == N):
        size = len(list(group))
        if is_n:
            runs.append((at, size))
        at += size
    return runs


def _counts(data):
    w = [0] * WORDS
    w[LEN] = len(data)
    for b in bytes(data):
        w[CLASS[b]] += 1
        if 0x61 <= b <= 0x7A:
            w[LOWER] += 1
    return w


def _close(w, length, min_gap):
    w[RUNS] += 1
    if length >= min_gap:
        w[GAPS] += 1
        w[GAP_BASES] += length
    w[LONGEST] = max(w[LONGEST], length)


def whole(data, min_gap=1):
    """the finalised census of a complete string: every run counts"""
    w = _counts(data)
    for _, length in n_runs(data):
        _close(w, length, min_gap)
    return w


def partial(data, min_gap=1):
    """the census of a piece: the runs that touch an end stay open in PRE / SUF"""
    w = _counts(data)
    n = len(data)
    for start, length in n_runs(data):
        if start == 0:
            w[PRE] = length
        if start + length == n:
            w[SUF] = length
        if start != 0 and start + length != n:
            _close(w, length, min_gap)
    return w


def merge(a, b, min_gap=1):
    if a[LEN] == 0:
        return list(b)
    if b[LEN] == 0:
        return list(a)
    out = [0] * WORDS
    for k in list(range(LEN, LOWER + 1)) + [RUNS, GAPS, GAP_BASES]:
        out[k] = a[k] + b[k]
    out[LONGEST] = max(a[LONGEST], b[LONGEST])
    all_a, all_b = a[PRE] == a[LEN], b[PRE] == b[LEN]
    out[PRE] = a[LEN] + b[PRE] if all_a else a[PRE]
    out[SUF] = a[SUF] + b[LEN] if all_b else b[SUF]
    if not all_a and not all_b and a[SUF] + b[PRE] > 0:
        _close(out, a[SUF] + b[PRE], min_gap)
    return out


def finalise(w, min_gap=1):
    out = list(w)
    if out[LEN] > 0 and out[PRE] == out[LEN]:
        _close(out, out[LEN], min_gap)
    else:
        for end in (PRE, SUF):
            if out[end] > 0:
                _close(out, out[end], min_gap)
    out[PRE] = out[SUF] = 0
    return out


def table(stream, seq_off, seq_len, min_gap=1, origin=0):
    """the partial census of every row over the whole ``stream`` (which begins at stream position ``origin``)"""
    return [partial(stream[o - origin:o - origin + n], min_gap) for o, n in zip(seq_off, seq_len)]


def windowed(stream, seq_off, seq_len, cuts, min_gap=1, origin=0, acc=None):
    """the protocol: windows [cuts[k], cuts[k + 1]) of the stream (positions relative to its first byte), each row's piece
    merged in as the right-hand neighbour; rows without bytes in a window are not touched"""
    acc = [[0] * WORDS for _ in seq_off] if acc is None else [list(r) for r in acc]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for i, (o, n) in enumerate(zip(seq_off, seq_len)):
            s, e = max(o - origin, lo), min(o - origin + n, hi)
            if e > s:
                acc[i] = merge(acc[i], partial(stream[s:e], min_gap), min_gap)
    return acc


def _reached(lengths, x):
    desc = sorted(lengths, reverse=True)
    total, running = sum(desc), 0
    for k, length in enumerate(desc):
        running += length
        if running * 100 >= x * total:
            return k, length
    return None


def nx(lengths, x):
    """None for no lengths"""
    hit = _reached(lengths, x)
    return None if hit is None else hit[1]


def lx(lengths, x):
    """0 for no lengths"""
    hit = _reached(lengths, x)
    return 0 if hit is None else hit[0] + 1


def split_fasta(text):
    """[(name, sequence bytes)] of a FASTA whose records are one header line and one sequence line (the scaffold file) or
    wrapped lines; plain Python"""
    out = []
    for line in bytes(text).split(b'\n'):
        if line.startswith(b'>'):
            out.append([line[1:].decode('ascii'), b''])
        elif out:
            out[-1][1] += line
    return [(name, seq) for name, seq in out]
