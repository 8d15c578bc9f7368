"""The integer-exact dot-product bound that the CPU tests of the references
share (tests/test_device_ref_cpu.py, tests/test_solveops_ref_cpu.py).

TEST INFRASTRUCTURE ONLY. Integers and exact fractions only: no rounded
floating-point operation takes part in the judgement.
"""
from fractions import Fraction


def exact(x):
    """A double as (integer, e) with x = integer / 2**e."""
    n, d = float(x).as_integer_ratio()
    return n, d.bit_length() - 1


def within_gamma(value, terms):
    """|value - sum of the exact products| <= gamma_k * sum |product| with
    gamma_k = k u / (1 - k u), u = 2^-53: the bound of a k-term dot product
    summed in any order (Higham, Accuracy and Stability, 3.1). The table's
    -0.0 case multiplies 1e-200 by -1e-200, which underflows, so the model
    with underflow applies: fl(a b) = a b (1 + d) + e with |e| <= 2^-1075
    (half the smallest subnormal; additions do not underflow), which adds
    k 2^-1075 / (1 - k u) to the bound -- nothing at the scale of any other
    value here. A term that is added without a product of its own is given as
    (term, 1.0)."""
    k = len(terms)
    prods = []
    for a, b in terms:
        (na, ea), (nb, eb) = exact(a), exact(b)
        prods.append((na * nb, ea + eb))
    vn, ve = exact(value)
    E = max([e for _, e in prods] + [ve, 1075])
    s = sum(n << (E - e) for n, e in prods)
    mag = sum(abs(n) << (E - e) for n, e in prods)
    err = abs((vn << (E - ve)) - s)
    return err * ((1 << 53) - k) <= k * mag + k * (1 << (E - 1075 + 53))


def is_one_rounding(value, a, b):
    """value == fl(a - b) under round-to-nearest-even: the exact rational
    difference, rounded once by Fraction.__float__ (an integer division that
    rounds correctly). An exact zero difference only asks for a zero."""
    diff = Fraction(float(a)) - Fraction(float(b))
    if diff == 0:
        return value == 0.0
    return float(diff) == value
