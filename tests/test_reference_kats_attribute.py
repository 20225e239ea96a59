"""Known-answer tests for the typed-attribute comparator, from the reference's
plugins/shared/structs/attribute_test.go (Compare_Bool 90-139, Compare_String
141-199, Compare_Float 201-250, Compare_Int 252-301, Compare_Int_With_Units
303-384, Compare_Float_With_Units 386-478, Compare_IntToFloat 480-529,
ParseAndValidate 544-666).

Device constraints and affinities (`${device.attr.memory} >= 40 GiB`) compare
typed attributes through Attribute.Compare. The tables run against the oracle
(oracle_check_attr) and the engine's host code (pe_check_attr in libnomadpe.so:
no GPU needed). The expected value of every row that the reference does not
state comes from `model_compare` below: a plain restatement of attribute.go:314-
460 on fractions.Fraction, with big.Float's 256-bit round-to-nearest-even written
out. Nothing expected here is taken from the code under test.
"""
import ctypes as C
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from nomad_amd import abi
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ENGINE = None


def engine_check_attr(op, left, r_text):
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = abi.bind_check_attr(C.CDLL(os.path.join(ROOT, "nomad_amd", "libnomadpe.so")))
    return abi.call_check_attr(_ENGINE.pe_check_attr, op, left, r_text)


CHECKERS = [pytest.param(oracle.check_attr, id="oracle"), pytest.param(engine_check_attr, id="engine-host")]

# ---- the reference model ------------------------------------------------------
# units.go: name -> (base, multiplier, inverse)
UNITS = {}
for _i, _p in enumerate(["KiB", "MiB", "GiB", "TiB", "PiB", "EiB"]):
    UNITS[_p] = ("byte", 1 << (10 * (_i + 1)), False)
    UNITS[_p + "/s"] = ("byterate", 1 << (10 * (_i + 1)), False)
for _p, _m in [("kB", 10 ** 3), ("KB", 10 ** 3), ("MB", 10 ** 6), ("GB", 10 ** 9), ("TB", 10 ** 12),
               ("PB", 10 ** 15), ("EB", 10 ** 18)]:
    UNITS[_p] = ("byte", _m, False)
    UNITS[_p + "/s"] = ("byterate", _m, False)
UNITS.update({"MHz": ("hertz", 10 ** 6, False), "GHz": ("hertz", 10 ** 9, False),
              "mW": ("watt", 10 ** 3, True), "W": ("watt", 1, False), "kW": ("watt", 10 ** 3, False),
              "MW": ("watt", 10 ** 6, False), "GW": ("watt", 10 ** 9, False)})

PREC = 256   # attribute.go:20 floatPrecision


def round_prec(x, prec=PREC):
    """big.Float's rounding (ToNearestEven) of an exact value to `prec` mantissa bits."""
    x = Fraction(x)
    if x == 0:
        return x
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()   # 2^e <= x < 2^(e+1), give or take one
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    ulp = Fraction(2) ** (e - prec + 1)
    q = x / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * n * ulp


def big_float(value, unit, prec=PREC):
    """getBigFloat (attribute.go:395-426), step by step."""
    f = round_prec(Fraction(value), prec)                # SetInt64 / SetFloat64
    if unit not in UNITS:
        return f
    _, mult, inverse = UNITS[unit]
    m = round_prec(Fraction(mult), prec)                 # multiplier.SetInt64
    if inverse:
        m = round_prec(Fraction(1) / m, prec)            # multiplier.Quo(base, multiplier)
    return round_prec(f * m, prec)                       # f.Mul(f, multiplier)


def _wrap64(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def get_int(value, unit):
    """getInt (attribute.go:430-456): int64 arithmetic, Go's truncating division."""
    if unit not in UNITS:
        return value
    _, mult, inverse = UNITS[unit]
    if inverse:
        q = abs(value) // mult
        return -q if value < 0 else q
    return _wrap64(value * mult)


def kind_of(v):
    return "bool" if isinstance(v, bool) else "int" if isinstance(v, int) else \
        "float" if isinstance(v, float) else "string"


def model_compare(a, b, prec=PREC):
    """Attribute.Compare (attribute.go:282-387) -> (v, comparable)."""
    (av, au), (bv, bu) = a, b
    ua, ub = UNITS.get(au), UNITS.get(bu)
    if ua and ub:
        if ua[0] != ub[0]:
            return 0, False
    elif ua or ub:
        return 0, False
    elif kind_of(av) == "string" and kind_of(bv) != "string":
        return 0, False
    elif kind_of(av) == "bool" and kind_of(bv) != "bool":
        return 0, False
    ka, kb = kind_of(av), kind_of(bv)
    if ka == "bool":
        return (0 if av == bv else 1), True
    if ka == "string":
        x, y = av.encode(), bv.encode()
        return (x > y) - (x < y), True
    if ka == "int" and kb == "int":
        x, y = get_int(av, au), get_int(bv, bu)
        return (x > y) - (x < y), True
    if kb not in ("int", "float"):
        return 0, False                                   # b.getBigFloat() == nil
    x, y = big_float(av, au, prec), big_float(bv, bu, prec)
    return (x > y) - (x < y), True


def model_check(op, a, b):
    """checkAttributeConstraint (feasible.go:1334-1447), both sides found."""
    v, ok = model_compare(a, b)
    if not ok:
        return False
    return {"=": v == 0, "==": v == 0, "is": v == 0, "!=": v != 0, "not": v != 0, "<": v == -1,
            "<=": v != 1, ">": v == 1, ">=": v != -1}[op]


def text_of(attr, sep=""):
    """The literal a jobspec would carry for a typed attribute (the right side is
    always parsed from text, as RTarget is)."""
    v, unit = attr
    sep = sep if unit else ""
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, float):
        s = repr(v)                  # shortest round-trip digits; always has '.', 'e', 'inf'
        assert float(s) == v
        return s + sep + unit
    if isinstance(v, int):
        return str(v) + sep + unit
    return v


OPS = ["=", "==", "is", "!=", "not", "<", "<=", ">", ">="]


def assert_row(check, a, b, sep=""):
    for op in OPS:
        want = model_check(op, a, b)
        got = check(op, a, text_of(b, sep))
        assert got == want, (op, a, b, text_of(b, sep), "want", want)


# ---- the reference's tables ----------------------------------------------------
# (A, B, expected Compare value; None = NotComparable)
def _rows(kind_rows):
    return [((a, au), (b, bu), want) for a, au, b, bu, want in kind_rows]


COMPARE_BOOL = _rows([          # attribute_test.go:90-139
    (True, "", True, "", 0), (True, "", False, "", 1), (True, "", "foo", "", None),
    (True, "", 123, "", None), (True, "", 123.2, "", None)])
COMPARE_STRING = _rows([        # :141-199
    ("a", "", "b", "", -1), ("hello", "", "hello", "", 0), ("b", "", "a", "", 1),
    ("hello", "", True, "", None), ("hello", "", 123, "", None), ("hello", "", 123.2, "", None)])
COMPARE_FLOAT = _rows([         # :201-250
    (101.5, "", 100001.5, "", -1), (100001.5, "", 100001.5, "", 0), (999999999.5, "", 101.5, "", 1),
    (101.5, "", True, "", None), (101.5, "", "hello", "", None)])
COMPARE_INT = _rows([           # :252-301
    (3, "", 10, "", -1), (10, "", 10, "", 0), (100, "", 10, "", 1), (10, "", True, "", None),
    (10, "", "hello", "", None)])
COMPARE_INT_UNITS = _rows([     # :303-384
    (3, "MB", 10, "MB", -1), (10, "MB", 10, "MB", 0), (100, "MB", 10, "MB", 1), (3, "GB", 3, "MB", 1),
    (1, "GiB", 1024, "MiB", 0), (1, "GiB", 1025, "MiB", -1), (1000, "mW", 1, "W", 0)])
COMPARE_FLOAT_UNITS = _rows([   # :386-478
    (3.0, "MB", 10.0, "MB", -1), (10.0, "MB", 10.0, "MB", 0), (100.0, "MB", 10.0, "MB", 1),
    (3.0, "GB", 3.0, "MB", 1), (1.0, "GiB", 1024.0, "MiB", 0), (1.0, "GiB", 1025.0, "MiB", -1),
    (1000.0, "mW", 1.0, "W", 0), (1.5, "GiB", 1400.0, "MiB", 1)])
COMPARE_INT_TO_FLOAT = _rows([  # :480-529
    (3, "", 10.0, "", -1), (10, "", 10.0, "", 0), (10, "", 10.1, "", -1), (100, "", 10.0, "", 1),
    (100, "", 100.00001, "", -1)])

TABLES = {"bool": COMPARE_BOOL, "string": COMPARE_STRING, "float": COMPARE_FLOAT, "int": COMPARE_INT,
          "int_with_units": COMPARE_INT_UNITS, "float_with_units": COMPARE_FLOAT_UNITS,
          "int_to_float": COMPARE_INT_TO_FLOAT}


@pytest.mark.parametrize("table", sorted(TABLES))
def test_model_gives_the_reference_tables(table):
    """The model itself against every value the reference states."""
    for a, b, want in TABLES[table]:
        v, ok = model_compare(a, b)
        assert (v if ok else None) == want, (a, b)


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("check", CHECKERS)
def test_compare_tables(check, table):
    """Every row of the seven Compare tables, seen through all nine operators:
    v == 0 is "=", v == -1 is "<", v == 1 is ">", not comparable is false for all."""
    for a, b, want in TABLES[table]:
        for op in OPS:
            if want is None:
                exp = False
            else:
                exp = {"=": want == 0, "==": want == 0, "is": want == 0, "!=": want != 0, "not": want != 0,
                       "<": want == -1, "<=": want != 1, ">": want == 1, ">=": want != -1}[op]
            for sep in ("", " "):
                assert check(op, a, text_of(b, sep)) == exp, (op, a, b, sep)


# attribute_test.go:544-666 TestAttribute_ParseAndValidate: input -> (value, unit)
PARSE = [("true", True, ""), ("false", False, ""), ("1", 1, ""), ("100", 100, ""), ("-100", -100, ""),
         ("-1.0", -1.0, ""), ("-100.25", -100.25, ""), ("1.01", 1.01, ""), ("100.25", 100.25, ""),
         ("foobar", "foobar", ""), ("foo123bar", "foo123bar", ""), ("100MB", 100, "MB"),
         ("-100MHz", -100, "MHz"), ("-1.0MB/s", -1.0, "MB/s"), ("-100.25GiB/s", -100.25, "GiB/s"),
         ("1.01TB", 1.01, "TB"), ("100.25mW", 100.25, "mW")]


@pytest.mark.parametrize("check", CHECKERS)
def test_parse_and_validate(check):
    """The literal parses to the expected kind, value and unit: "=" holds against
    that attribute, and fails against the same value of another kind or unit base
    ("1" is an Int, not the Bool strconv.ParseBool would also accept)."""
    for text, v, unit in PARSE:
        assert check("=", (v, unit), text), (text, v, unit)
        assert not check("!=", (v, unit), text), (text, v, unit)
        if isinstance(v, bool):
            assert check("!=", (not v, ""), text)
            assert not check("=", (1 if v else 0, ""), text)
            assert not check("=", ("true" if v else "false", ""), text)
        elif isinstance(v, str):
            assert not check("=", (v + "x", ""), text)
        else:
            assert not check("=", (str(v), ""), text), text            # a number, not a string
            assert check("<", (v - 1, unit), text) and check(">", (v + 1, unit), text), text
            other = "GHz" if UNITS.get(unit, ("", 0, 0))[0] != "hertz" else "GiB"
            assert not check("=", (v, other), text), (text, other)     # unit against none / another base
            assert not check("!=", (v, other), text), (text, other)
    assert not check("=", (True, ""), "1")
    assert check("=", (1, ""), "1")


# the same power in mW and in W (the one inverse unit): equal at 256 bits, "less" at 64
MILLIWATTS = [250, 500, 1000, 1500, 2000, 3000, 7000, 123000]


def test_model_inverse_unit_needs_256_bits():
    """v * round(1/1000) rounds back to v/1000 at 256 bits and falls short of it
    at 64 (a long double's mantissa): the reference's own row separates the two."""
    for mw in MILLIWATTS:
        a, b = (float(mw), "mW"), (mw / 1000.0, "W")
        assert model_compare(a, b) == (0, True), mw
        assert model_compare(a, b, prec=64) == (-1, True), mw


@pytest.mark.parametrize("check", CHECKERS)
def test_milliwatts_against_watts(check):
    """attribute_test.go:454-464 (Float 1000.0 mW == Float 1.0 W) and its kin,
    float/float and the mixed Int/Float pairs, both ways round."""
    for mw in MILLIWATTS:
        w = mw / 1000.0
        assert w * 1000.0 == mw
        for a, b in [((float(mw), "mW"), (w, "W")), ((w, "W"), (float(mw), "mW")),
                     ((mw, "mW"), (w, "W")), ((w, "W"), (mw, "mW"))]:
            assert model_compare(a, b) == (0, True)
            assert_row(check, a, b)
            assert_row(check, a, b, " ")
        if w == int(w):
            for a, b in [((float(mw), "mW"), (int(w), "W")), ((int(w), "W"), (float(mw), "mW"))]:
                assert model_compare(a, b) == (0, True)
                assert_row(check, a, b)
    # one mW more or less is seen
    assert check("<", (999.0, "mW"), "1.0 W") and check(">", (1001.0, "mW"), "1.0 W")
    assert check("<", (999, "mW"), "1.0 W") and check(">", (1001, "mW"), "1.0 W")
    # int/int stays on getInt's integer division: 1999 mW is 1 W
    assert check("=", (1999, "mW"), "1 W") and check(">", (1999, "mW"), "1.0 W")


def _next(x, k):
    """The float k places after x (k may be negative), x > 0."""
    return struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", x))[0] + k))[0]


PAIRS = [("GiB", "MiB"), ("GB", "MB"), ("EB", "PB"), ("W", "mW"), ("GHz", "MHz"), ("PiB", "KiB"), ("kW", "mW"),
         ("GW", "mW"), ("GiB/s", "MiB/s")]


def generated_pairs():
    """Seeded: the same quantity in two units of one base, as ints, floats and
    mixed, and float values next to each other in the last place."""
    rng = np.random.Generator(np.random.PCG64(20261021))
    out = []
    for big, small in PAIRS:
        ratio = Fraction(UNITS[big][1]) * (UNITS[small][1] if UNITS[small][2] else 1) / \
            (1 if UNITS[small][2] else UNITS[small][1])
        for _ in range(6):
            n = int(rng.integers(1, 4000))
            small_n = n * ratio
            assert small_n.denominator == 1
            small_n = int(small_n)
            if small_n >= 1 << 53:
                n, small_n = 1, int(ratio)
            for d in (-1, 0, 1):
                out.append(((n, big), (small_n + d, small)))
                out.append(((float(n), big), (float(small_n + d), small)))
                out.append(((float(n), big), (small_n + d, small)))
                out.append(((small_n + d, small), (float(n), big)))
            # fractional amounts of the larger unit, and their neighbours in the last place
            x = n + float(rng.integers(1, 1024)) / 1024.0
            y = float(x * float(ratio))
            for k in (-2, -1, 0, 1, 2):
                out.append(((x, big), (_next(y, k), small)))
                out.append(((_next(y, k), small), (x, big)))
    for _ in range(40):   # bare floats, neighbours in the last place, and ints near 2^53 .. 2^63
        x = float(rng.random() * 10.0 ** int(rng.integers(-8, 18)))
        for k in (-1, 0, 1):
            out.append(((x, ""), (_next(x, k), "")))
        i = int(rng.integers(1 << 53, (1 << 63) - 2))
        for d in (-1, 0, 1):
            out.append(((i + d, ""), (float(i), "")))
            out.append(((float(i), ""), (i + d, "")))
    return out


def test_generated_pairs_cover_all_three_answers():
    got = {model_compare(a, b)[0] for a, b in generated_pairs()}
    assert got == {-1, 0, 1}
    assert len(generated_pairs()) > 300


@pytest.mark.parametrize("check", CHECKERS)
def test_generated_pairs(check):
    for a, b in generated_pairs():
        assert_row(check, a, b)


@pytest.mark.parametrize("check", CHECKERS)
def test_wide_values(check):
    """Values whose product with the multiplier needs more than 64 bits, where a
    64-bit mantissa would round: still exact at 256."""
    big = (1 << 62) + 1
    rows = [((float(1 << 62), "EiB"), (big, "EiB")),          # mixed: 2^62 against 2^62 + 1, times 2^60
            ((big, "EB"), (float(1 << 62), "EB")),
            ((9007199254740993, "EB"), (9007199254740992.0, "EB")),   # 2^53 + 1 against 2^53
            ((1e300, "GW"), (_next(1e300, 1), "GW")),
            ((5e-324, "mW"), (0.0, "W")), ((-5e-324, "mW"), (0.0, "W")), ((0.0, "mW"), (-0.0, "W")),
            ((-3.5, "GiB"), (-3584.0, "MiB")), ((-3.5, "GiB"), (-3585, "MiB"))]
    for a, b in rows:
        assert_row(check, a, b)
        assert_row(check, b, a)
