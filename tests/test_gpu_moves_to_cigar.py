"""hs_moves_to_cigar alone (k_m2c_count / the scan / k_m2c_write, hs_kernels_realign.hip): synthetic move arrays in the layout
hs_edlib_hw_align leaves them -> packed CIGAR words, against a numpy restatement (the rule of tests/test_cpu_edlib_cigar.py's
_restated, STANDARD format, mapped to words). One call holds every pair, shuffled, so that the pairs start at arbitrary byte
offsets, their words at arbitrary word offsets, and a 65537-move pair lies between one-move pairs. Pairs of 65 x 1024 + 1 and 129 x 1024 + 1
moves end a run in the second and the third step of k_m2c_write's search (64 chunks a step); the fixture asserts that they do."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HS_EINVAL = -2
LENGTHS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 65537, 66561, 132097]
CLIPS = [(0, 0), (5, 0), (0, 7), (5, 7)]
CLASS = np.array([0, 1, 2, 0], np.uint32)      # moves 0 '=' and 3 'X' are M, 1 is I, 2 is D


def _restated_words(moves, n_moves, clip):
    """the words of one pair: <left clip>S, the runs of equal class as M / I / D, <right clip>S; nothing at all without moves"""
    if n_moves <= 0:
        return np.zeros(0, np.uint32), (0, 0)
    c = CLASS[np.asarray(moves[:n_moves], np.uint8)]
    starts = np.concatenate(([0], np.flatnonzero(c[1:] != c[:-1]) + 1))
    runs = np.diff(np.concatenate((starts, [len(c)]))).astype(np.uint32)
    w = [(runs << 4) | c[starts]]
    if clip[0] > 0:
        w.insert(0, np.array([(clip[0] << 4) | 4], np.uint32))
    if clip[1] > 0:
        w.append(np.array([(clip[1] << 4) | 4], np.uint32))
    spans = (int((c != 1).sum()), int((c != 2).sum()) + max(clip[0], 0) + max(clip[1], 0))
    return np.concatenate(w).astype(np.uint32), spans


def _boundaries(L, m, d):
    """moves whose class changes exactly at every k * m + d inside (0, L)"""
    cut = np.arange(m, L + 2, m) + d
    cut = cut[(cut > 0) & (cut < L)]
    run_of = np.searchsorted(cut, np.arange(L), side="right")
    return np.array([0, 1, 3, 2], np.uint8)[run_of % 4]      # M I M D ...: neighbours always differ in class


def _patterns(L, rng):
    yield "one class", np.full(L, [0, 1, 2, 3][L % 4], np.uint8)
    yield "I/D alternation", np.array([1, 2], np.uint8)[np.arange(L) % 2]
    yield "0 3 0 3", np.array([0, 3], np.uint8)[np.arange(L) % 2]
    k = L // 1 + 1
    yield "random runs", np.repeat(rng.integers(0, 4, size=k), rng.integers(1, 31, size=k)).astype(np.uint8)[:L]
    yield "long run + one", np.concatenate((np.full(L - 1, 3, np.uint8), [1])).astype(np.uint8)
    mid = rng.integers(0, 4, size=max(L - 2, 0)).astype(np.uint8)
    at = L - 1 - L // 8      # (L = 132097: chunk 112, lane 47 of the search's second step)
    yield "one later start", np.concatenate((np.full(at, 3, np.uint8), np.full(L - at, 1, np.uint8)))
    yield "I first, D last", (np.concatenate(([1], mid, [2])) if L >= 2 else np.array([1])).astype(np.uint8)


def _search_from_chunk_0(mv):
    """how k_m2c_write's search for the end of chunk 0's last run goes on a pair whose chunk 0 holds one start: (steps taken, the lane that holds the first
    later chunk with a start or None). Step s looks at the chunks 1 + 64 s .. 64 + 64 s."""
    c = CLASS[mv]
    starts = np.concatenate(([0], np.flatnonzero(c[1:] != c[:-1]) + 1))
    if (starts < 1024).sum() != 1:
        return None
    c_last = (len(mv) - 1) // 1024
    later = starts[starts >= 1024] // 1024
    if len(later) == 0:
        return len(range(1, c_last + 1, 64)), None
    return (int(later[0]) - 1) // 64 + 1, (int(later[0]) - 1) % 64


@pytest.fixture(scope="module")
def pairs():
    """[(name, moves array (the pair's room), ops_len, (clip left, clip right))] in the order of the call, and the restatement"""
    rng = np.random.default_rng(20240611)
    ps = []
    for L in LENGTHS:
        for name, mv in _patterns(L, rng):
            assert len(mv) == L, (name, L, len(mv))
            for clip in CLIPS:
                ps.append(("%s L=%d" % (name, L), mv, L, clip))
        k = 0
        for m in (16, 64, 256, 1024):
            for d in (-1, 0, 1):
                ps.append(("boundaries %d%+d L=%d" % (m, d, L), _boundaries(L, m, d), L, CLIPS[k % 4])); k += 1
    # the later steps of the search are reached: a start in chunk 0, none in the next 64 chunks, then the run's end at lane 0 of the second and of the third
    # step, at another lane of the second, and nowhere after two and after three steps
    search = {p[0]: _search_from_chunk_0(p[1]) for p in ps if p[2] > 65 * 1024}
    assert search["long run + one L=66561"] == (2, 0) and search["long run + one L=132097"] == (3, 0) and search["one later start L=132097"] == (2, 47)
    assert search["one class L=66561"] == (2, None) and search["one class L=132097"] == (3, None)
    order = rng.permutation(len(ps))
    ps = [ps[i] for i in order]
    junk = lambda n: rng.integers(0, 4, size=n).astype(np.uint8)
    # pairs without an alignment: first, in the middle, last; with and without room for moves
    ps.insert(0, ("first, ops_len -1", junk(70), -1, (5, 7)))
    mid = len(ps) // 2
    ps.insert(mid, ("middle, ops_len 0, no room", junk(0), 0, (5, 7)))
    ps.insert(mid, ("middle, ops_len -1", junk(2000), -1, (0, 0)))
    ps.append(("last, ops_len 0", junk(1030), 0, (5, 0)))
    want = [_restated_words(mv, n, clip) for _, mv, n, clip in ps]
    return ps, [w for w, _ in want], np.array([s for _, s in want], np.int32)


@pytest.fixture(scope="module")
def full_call(built, pairs):
    from hairsplitter_amd import api
    ps, _, _ = pairs
    return api.moves_to_cigar([p[1] for p in ps], clips=[p[3] for p in ps], spans=True, ops_len=[p[2] for p in ps])


def test_words_equal_the_restatement(pairs, full_call):
    ps, want, _ = pairs
    words, _ = full_call
    assert len(words) == len(ps)
    for p, w, g in zip(ps, want, words):
        assert len(g) == len(w) and np.array_equal(g, w), (p[0], p[3], g[:8], w[:8])
    for p, g in zip(ps, words):      # pairs without an alignment get no words at all, not even their clips
        if p[2] <= 0:
            assert len(g) == 0, p[0]


def test_spans_equal_the_sums_of_the_restatement(pairs, full_call):
    ps, _, want_spans = pairs
    _, spans = full_call
    bad = np.flatnonzero((spans != want_spans).any(axis=1))
    assert len(bad) == 0, [(ps[i][0], spans[i], want_spans[i]) for i in bad[:5]]


def test_count_only_gives_the_same_offsets_and_total(built, pairs):
    from hairsplitter_amd import api
    ps, want, want_spans = pairs
    off, spans = api.moves_to_cigar([p[1] for p in ps], clips=[p[3] for p in ps], spans=True, ops_len=[p[2] for p in ps], count_only=True)
    want_off = np.concatenate(([0], np.cumsum([len(w) for w in want])))
    assert np.array_equal(off, want_off)      # (word_off does not move across the pairs without an alignment)
    assert np.array_equal(spans, want_spans)


def test_one_pair_and_no_pair(built):
    from hairsplitter_amd import api
    mv = np.array([1, 0, 3, 0, 2, 2, 0], np.uint8)
    (w,) = api.moves_to_cigar([mv], clips=[(3, 0)])
    assert w.tolist() == [(3 << 4) | 4, (1 << 4) | 1, (3 << 4) | 0, (2 << 4) | 2, (1 << 4) | 0]
    (w,) = api.moves_to_cigar([mv])      # no clip arrays at all
    assert w.tolist() == [(1 << 4) | 1, (3 << 4) | 0, (2 << 4) | 2, (1 << 4) | 0]
    assert api.moves_to_cigar([]) == []
    assert api.moves_to_cigar([], count_only=True).tolist() == [0]
    # n == 0 is HS_OK whatever else is passed
    total = C.c_int64(-1)
    assert api.load().hs_moves_to_cigar(None, None, None, None, None, C.c_int32(0), None, None, C.c_int64(0), None, C.byref(total), None) == 0
    assert total.value == 0


def test_a_short_words_cap_is_refused_and_nothing_is_written(built, pairs):
    import torch
    from hairsplitter_amd import api
    lib = api.load()
    ps, want, _ = pairs
    sub = [i for i in range(len(ps)) if len(ps[i][1]) <= 4097][:200]
    mv = [ps[i][1] for i in sub]
    oo = np.zeros(len(sub) + 1, np.int64)
    np.cumsum([len(m) for m in mv], out=oo[1:])
    total_want = sum(len(want[i]) for i in sub)
    dev = "cuda:0"
    d_ops = torch.from_numpy(np.concatenate(mv)).to(dev)
    d_len = torch.tensor([ps[i][2] for i in sub], dtype=torch.int32, device=dev)
    d_cl = torch.tensor([ps[i][3][0] for i in sub], dtype=torch.int32, device=dev)
    d_cr = torch.tensor([ps[i][3][1] for i in sub], dtype=torch.int32, device=dev)
    d_off = torch.zeros(len(sub) + 1, dtype=torch.int64, device=dev)
    GUARD = 0x5EED5EED
    d_words = torch.full((total_want + 1,), GUARD, dtype=torch.int64, device=dev).to(torch.int32)      # the buffer and one guard word behind it
    total = C.c_int64(0)
    call = lambda cap: lib.hs_moves_to_cigar(api._p(d_ops), api._hp(oo, C.c_int64), api._p(d_len), api._p(d_cl), api._p(d_cr), C.c_int32(len(sub)), api._p(d_off),
                                             api._p(d_words), C.c_int64(cap), None, C.byref(total), None)
    assert call(total_want - 1) == HS_EINVAL
    assert total.value == total_want
    torch.cuda.synchronize()
    assert (d_words.cpu().numpy() == np.int32(GUARD)).all()      # refused before a word is written
    assert call(total_want) == 0
    torch.cuda.synchronize()
    got = d_words.cpu().numpy().view(np.uint32)
    assert got[total_want] == GUARD
    assert np.array_equal(got[:total_want], np.concatenate([want[i] for i in sub]))


def _refused(api, oo, n, msg):
    """a call of hs_moves_to_cigar that its host checks refuse before any launch: the message, n_words unwritten, the words' guard pattern whole"""
    import torch
    lib = api.load()
    dev = "cuda:0"
    d_ops = torch.zeros(64, dtype=torch.uint8, device=dev)      # (the refusal comes before anything reads a move)
    d_len = torch.ones(n, dtype=torch.int32, device=dev)
    d_off = torch.full((n + 1,), -3, dtype=torch.int64, device=dev)
    GUARD = 0x5EED5EED
    d_words = torch.full((64,), GUARD, dtype=torch.int64, device=dev).to(torch.int32)
    total = C.c_int64(-77)
    oo = np.ascontiguousarray(oo, np.int64)
    rc = lib.hs_moves_to_cigar(api._p(d_ops), api._hp(oo, C.c_int64), api._p(d_len), None, None, C.c_int32(n), api._p(d_off), api._p(d_words), C.c_int64(64), None, C.byref(total), None)
    assert rc == HS_EINVAL and lib.hs_last_error().decode() == msg
    torch.cuda.synchronize()
    assert total.value == -77 and (d_words.cpu().numpy() == np.int32(GUARD)).all() and (d_off.cpu().numpy() == -3).all()


def test_a_pair_with_room_for_2_to_the_28_moves_is_refused(built):
    from hairsplitter_amd import api
    _refused(api, [0, 10, 10 + (1 << 28), 20 + (1 << 28)], 3, "hs_moves_to_cigar: pair 1 has room for 268435456 moves (0 .. 2^28 - 1: the length field of a CIGAR word)")
    _refused(api, [0, 10, 9], 2, "hs_moves_to_cigar: pair 1 has room for -1 moves (0 .. 2^28 - 1: the length field of a CIGAR word)")


def test_more_than_2_to_the_31_chunks_are_refused(built):
    """rooms of 2^28 - 1 moves are 262144 chunks each: 8191 pairs stay below 2^31 - 4 chunks, the 8192nd passes it"""
    from hairsplitter_amd import api
    room = (1 << 28) - 1
    per = (room + 1023) // 1024
    assert 8191 * per <= 0x7fffffff - 4 < 8192 * per
    _refused(api, np.arange(8193, dtype=np.int64) * room, 8192, "hs_moves_to_cigar: more than 2^31 chunks of moves in one call")
