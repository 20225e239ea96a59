"""The fp64 scoring math on its own: gomath_dev.h (pow10_unit, pow10_go, exp_go,
log_go, fit_score), evict.inc's pow2_go, basic_distance and preemption_score,
and kernels.hip's order_key, run through pe_probe_math.

Three comparisons, none of them through a Select:

  * host build of the device header == the oracle's gomath.h, bit for bit (CPU);
  * the oracle == exact arithmetic (decimal, 60 digits) within the error the
    portable Go 1.16 algorithm itself shows on this input set (CPU). The bounds
    below are that measured maximum rounded up to a whole ulp; they exist to
    catch a constant mistyped in both restatements, which parity between them
    cannot see;
  * the gfx950 code object == the host build, bit for bit (GPU).

The input set is deterministic: the free fractions 1 - u/c a node can show, the
branch edges of the fast paths (y next to 0, 0.5 and 1, the NearZero cut of
exp, subnormal inputs and results) and the values outside (0, 1) where
pow10_go's loop and ldexp_go's subnormal branch run. Domain: pow10_* takes
finite y with |y| < 2^63, log_go takes x > 0 (both headers state it); a NaN
result (preemption_score's 0/0, exp_go(NaN)) compares as NaN.
"""
import ctypes as C
import decimal
import math
import os

import numpy as np
import pytest

from nomad_amd import abi
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nomad_amd", "libnomadpe.so")
PE_EHIP = -3

LN10 = 2.302585092994046
NEAR_ZERO = 2.0 ** -28
EXP_OVERFLOW = 7.09782712893383973096e+02
EXP_UNDERFLOW = -7.45133219101941108420e+02

# Max error of the oracle against exact arithmetic over the sets below, in ulps
# of the result (measured value beside each bound).
ULP_BOUND_POW10_UNIT = 3    # measured 2.866 at y = 0.5176900857107406 (34165 y in [0, 1])
ULP_BOUND_POW10_WIDE = 8    # measured 7.416 at y = 250.4428831014112 (4651 y, |y| <= 333)
ULP_BOUND_EXP_NET = 1       # measured 0.818 at x = -9.33855 (4800 x of preemptionScore's net-priority range)
ULP_BOUND_EXP = 1           # measured 0.886 (113127 x: every finite, non-zero result of the exp set)
ULP_BOUND_LOG = 1           # measured 0.752 (34043 x > 0)


# ---- the probe ----------------------------------------------------------------------

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = abi.bind_probes(C.CDLL(LIB))
    return _lib


def probe(op, x, device=0, expect=0):
    """pe_probe_math over float64 items (scalar ops) or int64 rows; returns the result bits."""
    if op in (abi.PE_PROBE_FIT_SCORE, abi.PE_PROBE_BASIC_DISTANCE):
        xi = np.ascontiguousarray(x, dtype=np.int64)
        n, xd_p, xi_p = xi.shape[0], None, xi.ctypes.data_as(abi.i64p)
    else:
        xd = np.ascontiguousarray(x, dtype=np.float64)
        n, xd_p, xi_p = len(xd), xd.ctypes.data_as(abi.f64p), None
    out = np.zeros(max(1, n), dtype=np.uint64)
    rc = lib().pe_probe_math(op, xd_p, xi_p, n, out.ctypes.data_as(abi.u64p), device)
    assert rc == expect, rc
    return out[:n]


def probe_pscore(sets, device=0):
    """pe_probe_math(PREEMPTION_SCORE) over a list of priority lists."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in sets] + [np.zeros(0, dtype=np.int64)])
    xi = np.ascontiguousarray(np.concatenate([off, flat]))
    out = np.zeros(max(1, len(sets)), dtype=np.uint64)
    rc = lib().pe_probe_math(abi.PE_PROBE_PREEMPTION_SCORE, None, xi.ctypes.data_as(abi.i64p), len(sets),
                             out.ctypes.data_as(abi.u64p), device)
    assert rc == 0, rc
    return out[:len(sets)]


def bits(values):
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, inputs):
    """Equal bit for bit; two NaNs compare equal whatever their payload."""
    g, w = got.view(np.float64), want.view(np.float64)
    bad = np.nonzero((got != want) & ~(np.isnan(g) & np.isnan(w)))[0]
    assert len(bad) == 0, [(inputs[i], hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


# ---- the input set ------------------------------------------------------------------

def neighbours(x, k=2):
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def _base_set():
    rng = np.random.Generator(np.random.PCG64(2024))
    v = [1.0 - u / c for c in range(1, 65) for u in range(c + 1)]
    for c in (3900, 4000, 7936, 8192, 65536, 2 ** 31 - 1):
        u = rng.integers(0, c + 1, size=2000)
        v += list(1.0 - u.astype(np.float64) / float(c))
    v += list(rng.integers(1, 2 ** 53, size=20000).astype(np.float64) / 2.0 ** 53)
    v += [0.0, -0.0, 1.0, 0.5, -0.5, 5e-324, 2.2250738585072014e-308, 1e-300, 1e-10]
    v += neighbours(0.5)[1:] + neighbours(1.0)[1:]
    v += neighbours(NEAR_ZERO / LN10, 3)   # y * log10 crosses exp's NearZero cut between these
    return np.array(v, dtype=np.float64)


BASE = _base_set()
POW10_WIDE = np.array([-0.25, -1, -2.5, 2, 3.75, 308, 308.3, 309, -323, -324, -400, 1e18, -1e18, 333, -333,
                       17.5, -17.5, 100.25, -307.9, -308.5, -315.75, -322.999], dtype=np.float64)
POW10_SET = np.concatenate([BASE, POW10_WIDE])


def _exp_net_set():
    """0.0048 * (net - 2048), net = max + sum / max as preemptionScore forms it:
    priorities 1..100, up to 1024 preempted allocs."""
    rng = np.random.Generator(np.random.PCG64(7))
    nets = [float(p) + float(p * k) / float(p) for p in range(1, 101) for k in (1, 2, 3, 31, 32, 33, 256, 1024)]
    for _ in range(4000):
        pr = rng.integers(1, 101, size=int(rng.integers(1, 1025)))
        nets.append(float(pr.max()) + float(pr.sum()) / float(pr.max()))
    return 0.0048 * (np.array(nets, dtype=np.float64) - 2048.0)


EXP_NET = _exp_net_set()


def _exp_set():
    v = list(BASE) + list(-BASE[::8]) + list(BASE * LN10) + list((BASE - 1.0) * LN10) + list(EXP_NET)
    for x in (NEAR_ZERO, -NEAR_ZERO, EXP_OVERFLOW, -EXP_OVERFLOW, EXP_UNDERFLOW):
        v += neighbours(x)
    v += list(np.linspace(-745.0, -708.0, 1481)) + [float(k) for k in range(-745, -707)]
    v += [-708.3964185322641, -709.0895657128241, 700.0, -700.0, 1.0, -1.0, 0.5 * math.log(2.0), 1.5 * math.log(2.0)]
    v += [np.nan, np.inf, -np.inf]
    return np.array(v, dtype=np.float64)


EXP_SET = _exp_set()
LOG_SET = np.concatenate([BASE[(BASE > 0)], [10.0, 2.0, math.sqrt(0.5), np.nextafter(math.sqrt(0.5), 0), 1e300,
                                             1.7976931348623157e308, 4.9e-320]])
POW2_SET = np.concatenate([BASE, -BASE, POW10_WIDE, [1e-170, 1e-200, -3e-162, 1e154, 1.4e154, -2e200, np.inf,
                                                     -np.inf, np.nan, 1.5e-154]])


def _fit_rows():
    """(cap_cpu, cap_mem, util_cpu, util_mem, spread) rows."""
    rng = np.random.Generator(np.random.PCG64(99))
    rows = []
    for c in range(1, 65):
        for u in range(c + 1):
            rows.append((c, 65 - c, u, (u * 7) % (66 - c)))
    for c in (3900, 4000, 7936, 8192, 65536, 2 ** 31 - 1):
        uc, um = rng.integers(0, c + 1, size=400), rng.integers(0, 8193, size=400)
        rows += [(c, 8192, int(a), int(b)) for a, b in zip(uc, um)]
        rows += [(4000, c, int(b) % 4001, int(a)) for a, b in zip(uc, um)]
    rows += [(4000, 8192, 4000, 8192), (4000, 8192, 0, 0), (4000, 8192, 2000, 4096), (4000, 8192, 4000, 0),
             (4000, 8192, 5000, 9000), (100, 100, 250, 1), (3, 3, 1, 2), (4000, 8192, 3999, 8191)]   # overcommitted too
    return np.array([r + (s,) for r in rows for s in (0, 1)], dtype=np.int64)


FIT_ROWS = _fit_rows()


def _distance_rows():
    """(ask cpu, mem, disk, alloc cpu, mem, disk) rows: zero asks (a skipped
    coordinate), allocs above and below the ask, equal to it (coordinate 0)."""
    rng = np.random.Generator(np.random.PCG64(5))
    rows = [(a, m, d, uc, um, ud) for a in (0, 1, 500) for m in (0, 256) for d in (0, 150)
            for uc in (0, 1, 500, 4000) for um in (0, 256, 8192) for ud in (0, 150, 300)]
    n = 6000
    ask = np.stack([rng.integers(0, 8001, size=n), rng.integers(0, 65537, size=n), rng.integers(0, 100001, size=n)], 1)
    got = np.stack([rng.integers(0, 8001, size=n), rng.integers(0, 65537, size=n), rng.integers(0, 100001, size=n)], 1)
    rows += [tuple(map(int, np.concatenate([a, g]))) for a, g in zip(ask, got)]
    rows += [(1, 1, 1, 2 ** 40, 2 ** 50, 2 ** 62), (2 ** 62, 2 ** 61, 2 ** 60, 0, 1, 3), (3, 3, 3, 1, 2, 4)]
    return np.array(rows, dtype=np.int64)


DIST_ROWS = _distance_rows()


def _priority_sets():
    rng = np.random.Generator(np.random.PCG64(17))
    sets = [[p] * k for p in (1, 50, 100) for k in (1, 2, 31, 32, 33, 255, 256)]
    for _ in range(1500):
        sets.append(list(rng.integers(1, 101, size=int(rng.integers(1, 257)))))
    sets += [[0], [0] * 5, [0] * 40, [], [0, 7, 0], [32000] * 256, [2047], [2048], [1, 2047]]
    return sets


PRIORITY_SETS = _priority_sets()


def _order_values():
    rng = np.random.Generator(np.random.PCG64(23))
    raw = rng.integers(0, 2 ** 64, size=1200, dtype=np.uint64).view(np.float64)
    raw = raw[np.isfinite(raw) & (raw != 0.0)][:1000]
    assert len(raw) == 1000
    mx, mn, sub = 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324
    return np.concatenate([[-np.inf, -mx, -1.0, -mn, -sub, sub, mn, 1.0, mx, np.inf], raw])


ORDER_VALUES = _order_values()

SCALAR_OPS = [("pow10_unit", abi.PE_PROBE_POW10_UNIT, POW10_SET), ("pow10_go", abi.PE_PROBE_POW10, POW10_SET),
              ("exp_go", abi.PE_PROBE_EXP, EXP_SET), ("log_go", abi.PE_PROBE_LOG, LOG_SET),
              ("pow2_go", abi.PE_PROBE_POW2, POW2_SET),
              ("order_key", abi.PE_PROBE_ORDER_KEY, np.concatenate([ORDER_VALUES, [0.0, -0.0], BASE[:2200]]))]
ROW_OPS = [("fit_score", abi.PE_PROBE_FIT_SCORE, FIT_ROWS), ("basic_distance", abi.PE_PROBE_BASIC_DISTANCE, DIST_ROWS)]


# ---- CPU: host build of the device header == the oracle -------------------------------

def test_input_set_reaches_the_branches():
    """The set holds what it claims: both sides of every cut the fast paths make."""
    y = POW10_SET
    assert (y * LN10 < NEAR_ZERO)[y > 0].any() and (y * LN10 >= NEAR_ZERO)[y > 0].any()
    assert ((y > 0.5) & (y < 1)).sum() > 10000 and ((y > 0) & (y < 0.5)).sum() > 10000
    for edge in (0.5, 1.0):
        assert np.nextafter(edge, 0) in y and np.nextafter(edge, 2) in y
    assert (y < 0).any() and (y > 1).any() and 5e-324 in y
    sub = oracle.go_exp(-740.0)
    assert 0.0 < sub < 2.2250738585072014e-308   # ldexp's subnormal branch
    assert 0.0 < oracle.go_pow(10.0, -315.75) < 2.2250738585072014e-308
    assert len(BASE) > 30000 and len(EXP_SET) > 30000


def test_pow10_equals_oracle():
    want = bits([oracle.go_pow(10.0, float(y)) for y in POW10_SET])
    assert_same_bits(probe(abi.PE_PROBE_POW10, POW10_SET), want, POW10_SET)
    assert_same_bits(probe(abi.PE_PROBE_POW10_UNIT, POW10_SET), want, POW10_SET)


def test_exp_equals_oracle():
    want = bits([oracle.go_exp(float(x)) for x in EXP_SET])
    assert_same_bits(probe(abi.PE_PROBE_EXP, EXP_SET), want, EXP_SET)


def test_log_equals_oracle():
    want = bits([oracle.go_log(float(x)) for x in LOG_SET])
    assert_same_bits(probe(abi.PE_PROBE_LOG, LOG_SET), want, LOG_SET)


def test_pow2_equals_oracle():
    want = bits([oracle.go_pow(float(x), 2.0) for x in POW2_SET])
    assert_same_bits(probe(abi.PE_PROBE_POW2, POW2_SET), want, POW2_SET)


def test_fit_score_equals_oracle():
    got = probe(abi.PE_PROBE_FIT_SCORE, FIT_ROWS)
    raw = np.array([oracle.score_fit(int(s), int(c), int(m), 0, 0, int(uc), int(um)) for c, m, uc, um, s in FIT_ROWS])
    assert_same_bits(got, bits(raw / 18.0), FIT_ROWS)   # the kernels keep the score over binPackingMaxFitScore


def test_fit_score_known_answers():
    """TestScoreFitBinPack's table (structs/funcs_test.go): a node with 2048 MHz
    and 4096 MB left after its reservation scores 18 / 0 (binpack / spread) when
    just filled, 0 / 18 when unutilized, 13.675 / 4.325 at half; the first two
    exactly. The kernels keep the score over binPackingMaxFitScore = 18."""
    rows = np.array([(2048, 4096, 2048, 4096, 0), (2048, 4096, 0, 0, 0), (2048, 4096, 2048, 4096, 1),
                     (2048, 4096, 0, 0, 1), (2048, 4096, 1024, 2048, 0), (2048, 4096, 1024, 2048, 1)], dtype=np.int64)
    got = probe(abi.PE_PROBE_FIT_SCORE, rows).view(np.float64)
    assert list(got[:4]) == [1.0, 0.0, 0.0, 1.0]
    assert abs(got[4] * 18.0 - 13.675) < 0.001 and abs(got[5] * 18.0 - 4.325) < 0.001
    # free = 0.5 on both dimensions: Pow's Sqrt case
    assert got[4] == (20.0 - 2 * math.sqrt(10.0)) / 18.0 and got[5] == (2 * math.sqrt(10.0) - 2) / 18.0


def test_basic_distance_equals_oracle():
    want = bits([oracle.basic_distance(*map(int, r)) for r in DIST_ROWS])
    assert_same_bits(probe(abi.PE_PROBE_BASIC_DISTANCE, DIST_ROWS), want, DIST_ROWS)


def test_preemption_score_equals_oracle():
    want = bits([oracle.preemption_score(s) for s in PRIORITY_SETS])
    got = probe_pscore(PRIORITY_SETS)
    assert_same_bits(got, want, PRIORITY_SETS)
    zero = [i for i, s in enumerate(PRIORITY_SETS) if not any(s)]
    assert len(zero) >= 4 and np.isnan(got.view(np.float64)[zero]).all() and np.isnan(want.view(np.float64)[zero]).all()
    # net priority 2047 + 2047 / 2047 = 2048 is the logistic's origin (rank.go:843)
    assert probe_pscore([[2047]]).view(np.float64)[0] == 0.5


def test_order_key_orders_as_less_than():
    v = ORDER_VALUES
    key = probe(abi.PE_PROBE_ORDER_KEY, v)
    lt = v[:, None] < v[None, :]
    assert (lt == (key[:, None] < key[None, :])).all()
    assert ((v[:, None] == v[None, :]) == (key[:, None] == key[None, :])).all()


def test_order_key_of_signed_zeros():
    """The keys of -0.0 and +0.0 differ (adjacent, -0.0 first) while Go's `>`
    calls them equal: the key is an order of scores only because no final score
    is -0.0."""
    k = probe(abi.PE_PROBE_ORDER_KEY, np.array([-0.0, 0.0]))
    assert int(k[0]) + 1 == int(k[1]) == 0x8000000000000000
    assert not (-0.0 < 0.0) and not (0.0 < -0.0)


def test_probe_rejects_bad_arguments_and_reports_no_device():
    import torch
    x = np.array([0.25])
    out = np.zeros(1, dtype=np.uint64)
    assert lib().pe_probe_math(99, x.ctypes.data_as(abi.f64p), None, 1, out.ctypes.data_as(abi.u64p), 0) == -1
    assert lib().pe_probe_math(abi.PE_PROBE_EXP, None, None, 1, out.ctypes.data_as(abi.u64p), 0) == -1
    too_wide = np.array([0, 257] + [1] * 257, dtype=np.int64)
    assert lib().pe_probe_math(abi.PE_PROBE_PREEMPTION_SCORE, None, too_wide.ctypes.data_as(abi.i64p), 1,
                               out.ctypes.data_as(abi.u64p), 0) == -1
    probe(abi.PE_PROBE_EXP, x, device=1, expect=0 if torch.cuda.is_available() else PE_EHIP)


# ---- CPU: the oracle against exact arithmetic ------------------------------------------

def max_ulp_error(fn, exact, xs):
    """max |fn(x) - exact(x)| in ulps of fn(x), over the finite non-zero results."""
    ctx = decimal.getcontext().copy()
    ctx.prec = 60
    ctx.Emax, ctx.Emin = decimal.MAX_EMAX, decimal.MIN_EMIN
    worst, at = decimal.Decimal(0), None
    for x in xs:
        r = fn(float(x))
        if r == 0.0 or not math.isfinite(r):
            continue
        err = abs(ctx.subtract(decimal.Decimal(r), exact(ctx, decimal.Decimal(float(x))))) / decimal.Decimal(math.ulp(r))
        if err > worst:
            worst, at = err, float(x)
    return float(worst), at


def d_pow10(ctx, y):
    return ctx.power(decimal.Decimal(10), y)


def test_oracle_pow10_unit_against_exact():
    ys = BASE[(BASE >= 0) & (BASE <= 1)]
    err, at = max_ulp_error(lambda y: oracle.go_pow(10.0, y), d_pow10, ys)
    print("Pow(10, y), y in [0, 1]: max %.3f ulp at y = %r over %d inputs" % (err, at, len(ys)))
    assert err <= ULP_BOUND_POW10_UNIT, (err, at)


def test_oracle_pow10_wide_against_exact():
    rng = np.random.Generator(np.random.PCG64(31))
    ys = np.concatenate([POW10_WIDE[np.abs(POW10_WIDE) <= 333], rng.uniform(-333.0, 333.0, size=4000),
                         np.arange(-323, 309).astype(np.float64)])
    err, at = max_ulp_error(lambda y: oracle.go_pow(10.0, y), d_pow10, ys)
    print("Pow(10, y), |y| <= 333: max %.3f ulp at y = %r over %d inputs" % (err, at, len(ys)))
    assert err <= ULP_BOUND_POW10_WIDE, (err, at)


def test_oracle_exp_against_exact():
    err, at = max_ulp_error(oracle.go_exp, lambda ctx, x: ctx.exp(x), EXP_NET)
    print("Exp, net-priority range: max %.3f ulp at x = %r over %d inputs" % (err, at, len(EXP_NET)))
    assert err <= ULP_BOUND_EXP_NET, (err, at)
    xs = EXP_SET[np.isfinite(EXP_SET)]
    err, at = max_ulp_error(oracle.go_exp, lambda ctx, x: ctx.exp(x), xs)
    print("Exp, the whole set: max %.3f ulp at x = %r over %d inputs" % (err, at, len(xs)))
    assert err <= ULP_BOUND_EXP, (err, at)


def test_oracle_log_against_exact():
    xs = LOG_SET[LOG_SET != 1.0]
    err, at = max_ulp_error(oracle.go_log, lambda ctx, x: ctx.ln(x), np.concatenate([xs, [10.0]]))
    print("Log, x > 0: max %.3f ulp at x = %r over %d inputs" % (err, at, len(xs) + 1))
    assert err <= ULP_BOUND_LOG, (err, at)


# ---- GPU: the gfx950 code object == the host build -------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,op,xs", SCALAR_OPS + ROW_OPS, ids=[o[0] for o in SCALAR_OPS + ROW_OPS])
def test_device_equals_host(name, op, xs):
    assert_same_bits(probe(op, xs, device=1), probe(op, xs, device=0), xs)


@pytest.mark.gpu
def test_device_preemption_score_equals_host():
    assert_same_bits(probe_pscore(PRIORITY_SETS, device=1), probe_pscore(PRIORITY_SETS, device=0), PRIORITY_SETS)
