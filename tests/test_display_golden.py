"""Pin the oracle's five display quantisers to the reference's own cell grids across screen sizes (tests/golden/display.npz,
tools/make_goldens_display.py): row lengths 2 .. 16380, screens from the smallest that draws one cell to 130 x 1100, widths at the
row length (every bin read, samples on the knots), history depths 1 .. 45, NaN / +-inf bins, a constant history."""
import numpy as np
import pytest

import display_cases as D

KINDS = ("wf", "ps", "gw", "sf", "sg")


def test_display_goldens_cover_the_geometry():
    cs = D.cases()
    for kind in KINDS:
        k = [c for c in cs if c.kind == kind]
        assert {c.length for c in k} >= {2, 3, 12, 60, 252, 1020, 4092, 16380}, kind
        assert min(c.disp_w for c in k) == (2 if kind == "sf" else 1), kind     # (the surface entry point's smallest screen is 4 x 10)
        assert min(c.disp_h for c in k) <= 1, kind
        assert any(c.disp_w >= 2 * c.length - 1 for c in k) and any(c.disp_w == c.length for c in k), kind
        assert any(np.isnan(c.rows).any() for c in k) and any(np.isposinf(c.rows).any() for c in k), kind
        assert any(np.isneginf(c.rows).any() for c in k), kind
    assert {len(c.rows) for c in cs if c.kind == "wf"} >= {1, 7, 30}
    assert {len(c.rows) for c in cs if c.kind == "ps"} >= {1, 7, 10}
    # the reference raises for a constant waterfall history (int(NaN)): the case is recorded as raised, and only there
    assert sorted((c.kind, c.length) for c in cs if c.raised) == [("wf", 12), ("wf", 1020)]


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_quantisers_draw_the_reference_cells(kind):
    bad = []
    for c in D.cases():
        if c.kind != kind or c.raised:
            continue
        a, b, rg = D.oracle(c)
        if not np.array_equal(a, c.a):
            bad.append(f"{c.name()}: a: {D.first_diff(a, c.a)}")
        if c.b is not None and not np.array_equal(b, c.b):
            bad.append(f"{c.name()}: b: {D.first_diff(b, c.b)}")
        if kind == "sg":
            assert np.allclose(rg, c.sg_range, rtol=1e-14, atol=0), c.name()
    assert not bad, "\n".join(bad[:20])
