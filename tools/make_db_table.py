#!/usr/bin/env python3
"""Table and constants of pss_db_exact.h (db64_core): for the 128 centres c_i = 1 + i / 128 the double nearest 1 / c_i and
10 log10 of THAT double's reciprocal (evaluated in x87 extended precision, then rounded), so that
10 log10 z = 10 log10(z * invc) + tab.y holds without the table's rounding; entry 0 is {1, 0} exactly.  Then the polynomial's
coefficients (-1)^(k+1) (10 / ln 10) / k and 10 log10 2.
    python tools/make_db_table.py > table.txt"""
import numpy as np

ld = np.longdouble
assert np.finfo(ld).nmant >= 63, "needs an extended-precision long double"
for i in range(128):
    c = 1.0 + i / 128.0
    invc = np.float64(1.0) / np.float64(c)
    logc = ld(0) if i == 0 else -ld(10) * np.log10(ld(invc))
    print("    {%s, %s}," % (float(invc).hex(), float(np.float64(logc)).hex()))
K = ld(10) / np.log(ld(10))
for k in range(1, 7):
    print("A%d" % k, float(np.float64((-1) ** (k + 1) * K / k)).hex())
print("10LOG10_2", float(np.float64(ld(10) * np.log10(ld(2)))).hex())
