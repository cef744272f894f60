"""The work-buffer layouts of the allele and the recruit table (hs_group_alleles_layout, hs_group_recruit_layout: no device needed) against a
restatement of the part order and the rounding rule: every part begins 256-byte aligned and takes at least 4 bytes."""
import ctypes as C

import pytest

HS_EINVAL = -2
SCAN_TILE = 4096                    # HS_SCAN_TILE: ints per tile of the exclusive scan; 16 bytes of scratch per tile
SLABS = 64 * 65536 * 4              # HS_ALLELE_WIDE_BLOCKS slabs of HS_ALLELE_WIDE_KEYS keys
SIZES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (4096, 4096, 4096), (4097, 4095, 4097), (3, 70_000, 1_000_003)]


def _parts(sizes, at=0):
    """offsets of parts of these sizes one after the other from `at`, and where the next part would begin"""
    offs = []
    for n in sizes:
        offs.append(at)
        at = (at + max(n, 4) + 255) & ~255
    return offs, at


def _tiles(n):
    return max((n + SCAN_TILE - 1) // SCAN_TILE, 1) * 16


def allele_layout(S, W, n):
    public, internal = _parts([S * 4, W * 4, W * 4, W * 4, (S + 1) * 8, (W + 1) * 8, S * 4, n * 4, n * 4])
    _, total = _parts([W * 4, S * 4, _tiles(max(S, W)), 4, S * 4, SLABS], internal)      # has_snp, n_cells, tile scratch, wide counter and list, slabs
    return dict(zip(("snp_win", "grp_n", "win_snp_first", "win_snp_last", "cell_off", "grp_off", "n_calls", "grp_ids", "grp_pack"), public), internal=internal, total_bytes=total)


def recruit_layout(S, W, n):
    a = allele_layout(S, W, n)
    (flag,), internal = _parts([n * 4], a["total_bytes"])
    (_, row_idx, ctr_off, win_row_off, status, _), total = _parts([n * 4, (n + 1) * 8, (n + 1) * 8, (W + 1) * 8, 4, _tiles(n)], internal)      # ctr_n in front, tile scratch behind
    return a, dict(flag=flag, row_idx=row_idx, ctr_off=ctr_off, win_row_off=win_row_off, status=status, internal=internal, total_bytes=total)


def _fields(s):
    return {k: int(getattr(s, k)) for k, _ in s._fields_ if k != "alleles"}


@pytest.mark.parametrize("S,W,n", SIZES)
def test_layouts_follow_the_part_order_and_the_rounding_rule(built, S, W, n):
    from hairsplitter_amd import api
    lib = api.load()
    A, R = api.AlleleLayout(), api.RecruitLayout()
    assert lib.hs_group_alleles_layout(C.c_int32(S), C.c_int32(W), C.c_int64(n), C.byref(A)) == 0
    assert lib.hs_group_recruit_layout(C.c_int32(S), C.c_int32(W), C.c_int64(n), C.byref(R)) == 0
    want_a, want_r = recruit_layout(S, W, n)
    assert _fields(A) == want_a == allele_layout(S, W, n)
    assert _fields(R.alleles) == want_a and _fields(R) == want_r
    assert all(v % 256 == 0 for v in list(want_a.values()) + list(want_r.values()))


def test_bad_arguments_are_refused(built):
    from hairsplitter_amd import api
    lib = api.load()
    A, R = api.AlleleLayout(), api.RecruitLayout()
    for fn, out in ((lib.hs_group_alleles_layout, A), (lib.hs_group_recruit_layout, R)):
        assert fn(C.c_int32(1), C.c_int32(1), C.c_int64(1), None) == HS_EINVAL
        for S, W, n in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
            assert fn(C.c_int32(S), C.c_int32(W), C.c_int64(n), C.byref(out)) == HS_EINVAL
    # the recruit table scans its labels with 32-bit counts: one tile below 2^31 is the most it takes; the allele table takes more
    most = 0x7fffffff - SCAN_TILE
    assert lib.hs_group_recruit_layout(C.c_int32(0), C.c_int32(0), C.c_int64(most), C.byref(R)) == 0
    assert lib.hs_group_recruit_layout(C.c_int32(0), C.c_int32(0), C.c_int64(most + 1), C.byref(R)) == HS_EINVAL
    assert lib.hs_group_alleles_layout(C.c_int32(0), C.c_int32(0), C.c_int64(most + 1), C.byref(A)) == 0
