"""The narrow exp's table position, restated in exact rational arithmetic (csrc/mcr_math.h: fexp<., NARROW>, kExpNarrowShift,
load_math_tables<ROTATED>; DESIGN.md "growth forms", bit 0).

The general form adds the shifter S = 1.5 2^52 to x 512/ln 2 in one FMA: the sum is rounded half to even onto the unit grid of
[2^52, 2^53), its low word is k and sum - S is k as a double.  The narrow form adds S + 256 instead and reads the low word of the
sum as the position k + 256 of a table loaded ROTATED, with no mask.  Three claims carry that, and each is checked here without
floating point: the biased sum is the unbiased sum + 256 for every product the window can give, exact ties included; its low
word is k + 256, in [0, 511]; and position k + 256 of the rotated table holds the value the centred layout of the parent form
kept at k & 511."""

from __future__ import annotations

import math
import os
import re
from fractions import Fraction

from conftest import REPO

CSRC = os.path.join(REPO, "monte_carlo_retirement_amd", "csrc")
S = 3 * 2**51                 # 1.5 * 2^52
BIAS = 256
STEP = math.log(2.0) / 512.0
# residues of x 512 / ln 2 around k: the centre, interior points, a hair inside either end of the reduction interval
RESIDUES = (0.0, -0.25, 1.0 / 3.0, 0.125, -0.5 + 1e-7, 0.5 - 1e-7, -0.5 + 1e-12, 0.5 - 1e-12)


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _exp_scale():
    m = re.search(r"constexpr double kExpScale = (0x[0-9a-fp.+-]+);", _source("mcr_tables.h"))
    return float.fromhex(m.group(1))


def round_half_even(q: Fraction) -> int:
    """q rounded onto the unit grid as an FMA's single rounding does it: to nearest, ties to the even integer."""
    f = math.floor(q)
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        return f + 1
    return f


def on_the_unit_grid(n: int) -> bool:
    return 2**52 <= n < 2**53                # every integer there is a double, and the doubles there are the integers


def low_word(n: int) -> int:
    """The low 32 bits of the double n in [2^52, 2^53): its fraction field is n - 2^52, and 2^52 is a multiple of 2^32."""
    assert on_the_unit_grid(n)
    return n & 0xFFFFFFFF


def _products():
    """(k, exact product x c) for doubles x across the whole window, and synthetic exact ties k +- 1/2 (a product of two doubles
    rarely is one; the FMA rounds whatever it is given once, so the claim has to hold for them too)."""
    c = Fraction(_exp_scale())
    for k in range(-256, 256):
        for f in RESIDUES:
            x = (k + f) * STEP
            yield k, Fraction(x) * c
        for tie in (Fraction(-1, 2), Fraction(1, 2)):
            yield k, Fraction(k) + tie


def test_the_constants_are_the_ones_restated_here():
    math_h = _source("mcr_math.h")
    assert float(re.search(r"constexpr double kExpShift = ([0-9.]+);", math_h).group(1)) == float(S)
    assert re.search(r"constexpr double kExpNarrowShift = kExpShift \+ \(double\)\(1 << \(kExp2Bits - 1\)\);", math_h)
    assert re.search(r"constexpr int kExp2Bits = 9;", _source("mcr_tables.h"))
    assert S % 2 == 0 and (S + BIAS) % 2 == 0            # both shifters are even: a tie sees the same parity
    assert float(S + BIAS) == S + BIAS                   # (and the biased one is a double)
    assert abs(_exp_scale() - 512.0 / math.log(2.0)) < 1e-12


def test_the_biased_sum_is_the_unbiased_sum_plus_256():
    n = ties = 0
    for k, prod in _products():
        plain = round_half_even(prod + S)
        biased = round_half_even(prod + S + BIAS)
        assert on_the_unit_grid(plain) and on_the_unit_grid(biased), k
        assert biased == plain + BIAS, (k, prod)
        # kf = sum - shifter, exact in both forms (an integer below 2^9): the same double, so r and the polynomial are too
        assert biased - (S + BIAS) == plain - S
        n += 1
        ties += (prod + S).denominator == 2
    assert n == 512 * (len(RESIDUES) + 2) and ties == 2 * 512


def test_the_low_word_of_the_biased_sum_is_the_position():
    seen = set()
    for k, prod in _products():
        plain = round_half_even(prod + S)
        kk = plain - S                                   # the k the kernel works with (at a tie: the even neighbour)
        if not -256 <= kk <= 255:
            assert prod == Fraction(511, 2), (k, prod)   # the tie at the window's upper end goes to 256: outside (-256.5 goes to -256)
            continue
        assert low_word(plain) == kk & 0xFFFFFFFF        # the general form: k in two's complement, masked with 511 for the index
        p = low_word(round_half_even(prod + S + BIAS))
        assert p == kk + BIAS and 0 <= p <= 511, (k, prod, p)
        seen.add(p)
    assert seen == set(range(512))


def _centred(entries):
    """The parent form's layout: entry j is 2^(j/512), halved for j >= 256; k reads entry k & 511."""
    return [(j, j >= 256) for j in entries]


def _rotated(entries):
    """load_math_tables<ROTATED>: position p takes entry p ^ 256 and halves it for p < 256."""
    return [(p ^ 256, p < 256) for p in entries]


def test_the_rotated_position_names_the_value_the_centred_layout_gave():
    centred, rotated = _centred(range(512)), _rotated(range(512))
    for k in range(-256, 256):
        j, halved = rotated[k + BIAS]
        assert (j, halved) == centred[k & 511], k
        # and that value is 2^(k/512): entry j = k mod 512, times 1/2 exactly when k < 0
        assert j == k % 512 and halved == (k < 0)
        assert Fraction(j, 512) - (1 if halved else 0) == Fraction(k, 512)
    assert sorted(j for j, _ in rotated) == list(range(512))           # every entry is used once: same size, same LDS


def test_the_loader_in_the_source_is_the_one_restated_here():
    math_h = _source("mcr_math.h")
    assert "kMathTab[rot ? kTabExp2 + ((i - kTabExp2) ^ kHalf) : i]" in math_h
    assert "(rot && i < kTabExp2 + kHalf) ? 0.5 * v : v" in math_h
    assert "NARROW ? tab[kTabExp2 + (uint32_t)k]" in math_h
