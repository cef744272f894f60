"""2x2 tables at the chi-square thresholds of keep_only_robust_variants (loop C: > 15, loop D: > 20; call_variants.cpp:721-764), and a
step-by-step numpy restatement of computeChiSquare (:1135-1163) -- float margins and expectations, double squares, a float sum."""
import numpy as np


def exact_tables(thr, max_total=255):
    """every (n00, n01, n10, n11) with total <= max_total whose chi-square is exactly thr in exact arithmetic:
    N * det^2 == thr * r1 * (N - r1) * c1 * (N - c1), with det = n11 * n00 - n10 * n01 = N * n11 - r1 * c1"""
    out = []
    for N in range(2, max_total + 1):
        r1, c1 = np.meshgrid(np.arange(1, N, dtype=np.int64), np.arange(1, N, dtype=np.int64), indexing="ij")
        k = thr * r1 * (N - r1) * c1 * (N - c1)
        ok = k % N == 0
        s2 = np.where(ok, k // N, 0)
        s = np.round(np.sqrt(s2.astype(np.float64))).astype(np.int64)
        for d in (-1, 0, 1):      # (exact integer square root around the float one)
            ok_s = ok & ((s + d) * (s + d) == s2)
            for sign in (1, -1):
                num = r1 * c1 + sign * (s + d)      # N * n11
                sel = ok_s & (num % N == 0) & (s + d > 0)
                n11 = num // N
                sel &= (n11 >= np.maximum(0, r1 + c1 - N)) & (n11 <= np.minimum(r1, c1))
                for a, b, c in zip(r1[sel], c1[sel], n11[sel]):
                    out.append((int(N - a - b + c), int(b - c), int(a - c), int(c)))
    return sorted(set(out))


def exact_chi(t):
    """chi-square of tables [k, 4] (n00, n01, n10, n11) as a float64 of the exact rational value"""
    t = np.asarray(t, np.int64)
    n = t.sum(1); r1 = t[:, 2] + t[:, 3]; c1 = t[:, 1] + t[:, 3]
    det = n * t[:, 3] - r1 * c1
    return n * det.astype(np.float64) ** 2 / (r1 * (n - r1) * c1 * (n - c1)).astype(np.float64)


def near_tables(thr, k, rng, window=0.06, max_total=255):
    """k random tables (total <= max_total, every margin non-zero) whose exact chi-square lies within `window` of thr"""
    got = []
    while sum(len(g) for g in got) < k:
        t = rng.integers(0, 80, (400_000, 4))
        t = t[(t.sum(1) <= max_total) & (t[:, 2] + t[:, 3] > 0) & (t[:, 0] + t[:, 1] > 0) & (t[:, 1] + t[:, 3] > 0) & (t[:, 0] + t[:, 2] > 0)]
        chi = exact_chi(t)
        got.append(t[(np.abs(chi - thr) < window) & (chi != thr)])
    return [tuple(int(x) for x in r) for r in np.concatenate(got)[:k]]


def chi_square_reference(n00, n01, n10, n11):
    """computeChiSquare (call_variants.cpp:1135-1163) operation by operation: float / int divisions, float products, the four differences
    rounded to float and then squared and divided in double, the sum rounded to float"""
    f = np.float32
    n = n00 + n01 + n10 + n11
    if n == 0:
        return f(0)
    fn = f(n)
    p1 = f(n10 + n11) / fn
    p2 = f(n01 + n11) / fn
    one = f(1)
    if p1 * (one - p1) == 0 and p2 * (one - p2) == 0:
        return f(-1)
    if p1 * p2 * (one - p1) * (one - p2) == 0:
        return f(0)
    e00 = (one - p1) * (one - p2) * fn; e01 = (one - p1) * p2 * fn
    e10 = p1 * (one - p2) * fn; e11 = p1 * p2 * fn
    d = [np.float64(f(f(x) - e)) for x, e in ((n00, e00), (n01, e01), (n10, e10), (n11, e11))]
    e = [np.float64(x) for x in (e00, e01, e10, e11)]
    s = d[0] * d[0] / e[0] + d[1] * d[1] / e[1] + d[2] * d[2] / e[2] + d[3] * d[3] / e[3]
    return f(s)


def _valid_pair(rng):
    """a reference code and a second code in 33..157 that pass the central-base test of loops A / D (call_variants.cpp:527-528, :751-752)"""
    while True:
        k0, k1 = (int(x) for x in rng.choice(np.arange(33, 128), 2, replace=False))
        if k0 % 5 != k1 % 5 and ((k1 - 33) % 5 != 4 or (k1 // 5 % 5 != k0 % 5 and k1 // 25 % 5 != k0 % 5)):
            return k0, k1


def table_case(seed=1):
    """Columns with prescribed 2x2 tables against one partition per contig (reads 0..254: state +1, 255..509: -1, 510..: outside = 2), for
    K4 and its oracle. Every exact-threshold table with total <= 255, a few hundred tables near each threshold, loop C's 2 * total = n, n +- 1
    and loop D's 4 / 5 reads per side; 15-tables go to loop C (candidates), 20-tables to loop D (not candidates). Each table is laid out
    in three ways: two codes and n <= 255 where it fits (k_column_partition_lanes), a third code as frequent as the second within the
    partition (k_column_partition_grouped), and n > 255 or a reference code >= 128 (k_column_partition_test). Plus four columns of about
    200 entries side by side (more than a wavefront's 512 LDS entries in the first kernel). Returns (case, n_reads, table, route)."""
    rng = np.random.default_rng(seed)
    A, B, X = 255, 255, 300
    N = A + B + X
    plus, minus, out_ = np.arange(A), np.arange(A, A + B), np.arange(A + B, N)
    specs = []      # (table, loop, extra entries outside the partition, route)
    for thr, loop in ((15, "C"), (20, "D")):
        tabs = exact_tables(thr) + near_tables(thr, 300, rng)
        for t in tabs:
            T = sum(t)
            for route in ("lanes", "grouped", "test"):
                e = 0
                if route == "test":
                    e = max(0, 256 - T) if (loop == "D" or T > 128) else 0
                specs.append((t, loop, e, route))
    for T in (60, 100, 127):      # loop C's 2 * total against the column size n: n = 2T - 1, 2T, 2T + 1
        t = next(x for x in exact_tables(15, 127) if sum(x) == T) if any(sum(x) == T for x in exact_tables(15, 127)) else (T // 4, T // 4, T // 4, T - 3 * (T // 4))
        for e in (T - 1, T, T + 1):
            specs.append((t, "C", e, "lanes"))
    for t in ((0, 100, 5, 0), (0, 100, 4, 0), (5, 0, 0, 100), (4, 0, 0, 100), (2, 60, 3, 0), (40, 3, 1, 40)):      # loop D: 4 / 5 reads per side
        specs.append((t, "D", 0, "lanes")); specs.append((t, "D", 0, "grouped"))
    for _ in range(4):      # four wide columns in a row
        specs.append(((50, 50, 50, 50), "C", 0, "lanes"))
    col_off = [0]; col_idx = []; col_code = []; k0s = []; k1s = []; c1s = []; cand = []; tables = []; routes = []
    for t, loop, e, route in specs:
        n00, n01, n10, n11 = t
        k0, k1 = _valid_pair(rng)
        if route == "test" and sum(t) + e <= 255:
            k0 += 128 - 33 if k0 + 128 - 33 <= 255 else 0      # (no room for n > 255: a reference code >= 128 instead)
        k2 = next(k for k in range(33, 158) if k not in (k0, k1))
        third = route == "grouped"
        need_p = n11 + n10 * (2 if third else 1)
        need_m = n01 + n00 * (2 if third else 1)
        if need_p > A or need_m > B or e > X:
            continue
        ip = np.sort(rng.choice(plus, need_p, replace=False)); im = np.sort(rng.choice(minus, need_m, replace=False))
        cp = rng.permutation(np.array([k0] * n11 + [k1] * n10 + ([k2] * n10 if third else []), np.int64))
        cm = rng.permutation(np.array([k0] * n01 + [k1] * n00 + ([k2] * n00 if third else []), np.int64))
        ix = np.sort(rng.choice(out_, e, replace=False))
        cx = np.full(e, k0, np.int64)
        idx = np.concatenate((ip, im, ix)); code = np.concatenate((cp, cm, cx))
        col_idx.append(idx); col_code.append(code); col_off.append(col_off[-1] + len(idx))
        k0s.append(k0); k1s.append(k1); c1s.append(n10 + n00); cand.append(1 if loop == "C" else 0)
        tables.append(t); routes.append(route)
    n = len(k0s)
    case = dict(col_off=np.array(col_off, np.int64), col_idx=np.concatenate(col_idx).astype(np.int32), col_code=np.concatenate(col_code).astype(np.uint8),
                col_contig=np.zeros(n, np.int32), col_k0=np.array(k0s, np.uint8), col_k1=np.array(k1s, np.uint8), col_c1=np.array(c1s, np.int32),
                col_is_cand=np.array(cand, np.uint8), part_off=np.array([0, 1], np.int32), part_state_off=np.array([0], np.int64),
                part_state=np.concatenate((np.ones(A), -np.ones(B), np.full(X, 2))).astype(np.int8))
    return case, [N], np.array(tables, np.int64), np.array(routes)
