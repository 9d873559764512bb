"""-m gpu : the open-set solve (include/k16.h k16_r1cs_open_system / k16_r1cs_open_direction; csrc/r1cs_scan.hip
k_r1cs_open_rref, csrc/r1cs_open.h) against the big-integer reference of tests/open_system_reference.py.  Every case compares the
counts, the list, the class and the component of every wire, and the component's sizes, the rank and the direction of every wire
that is neither FIXED nor ABSENT, byte for byte with the reference; every case runs twice for equal bytes; and for each FREE
wire the direction is added to the witness and the check must find no constraint broken that it did not find broken before
(none at all on a satisfied circuit).  What each directed
circuit's classes must be is asserted of the reference itself in tests/test_open_system_host.py."""
import ctypes as C

import numpy as np
import pytest

import open_system_reference as osr
import r1cs_builder as rb
from open_system_reference import ABSENT, FIXED, FORCED, FREE, SKIPPED, UNDECIDED, R

pytestmark = pytest.mark.gpu

ERR_ARG = -3


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def snapshot(circ, c, asked):
    """everything both calls report, in a form that compares byte for byte"""
    s = circ.open_system(c["fixed"], want_maps=True)
    out = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    out["directions"] = {x: circ.open_direction(c["fixed"], x) for x in asked}
    return s, out


def assert_case(ctx, c, res, what=None, others=1):
    """check, both calls twice, against the reference; then every FREE direction through the check.  The direction call is made
    for every FREE wire and for every `others`-th wire of the remaining listed ones."""
    import k16
    n_wires, rowsA, rowsB, rowsC = c["circuit"]
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        base = rb.witness_bytes(c["w"])
        n_failed, failed = circ.check(base)
        assert failed.tolist() == res["broken"], what
        rest = [x for x in res["listed"] if res["classes"][x] != FREE]
        asked = sorted({x for x in res["listed"] if res["classes"][x] == FREE} | set(rest[::others] + rest[-1:]))
        s, first = snapshot(circ, c, asked)
        again = [x for x in asked if res["classes"][x] == FREE or len(asked) <= 16]       # the second run: every map, every FREE direction
        s2, second = snapshot(circ, c, again)
        assert {k: v for k, v in second.items() if k != "directions"} == {k: v for k, v in first.items() if k != "directions"}, what
        assert second["directions"] == {x: first["directions"][x] for x in again}, what   # the same bytes on every run
        for k in ("n_forced", "n_free", "n_undecided", "n_skipped", "n_absent", "n_components", "n_dims"):
            assert s[k] == res[k], (what, k)
        assert s["status"].tolist() == res["classes"], what
        assert s["comp"].tolist() == res["comp"], what
        assert s["wires"].tolist() == res["listed"] and s["classes"].tolist() == [res["classes"][x] for x in res["listed"]], what
        for x in asked:
            got, k = first["directions"][x], res["comps"][res["comp"][x]]
            assert got["cls"] == res["classes"][x], (what, x)
            assert (got["comp_wires"], got["comp_rows"], got["comp_cross"]) == (len(k["wires"]), len(k["rows"]), k["cross"]), (what, x)
            assert got["rank"] == (0 if k["skipped"] else k["rank"]), (what, x)
            assert got["d"] == osr.direction(res, x), (what, x)
        for x in [0] + [i for i, k in enumerate(res["classes"]) if k in (FIXED, ABSENT)][:3]:
            got = circ.open_direction(c["fixed"], x)
            assert (got["cls"], got["comp_wires"], got["comp_rows"], got["comp_cross"], got["rank"], got["d"]) == \
                (res["classes"][x], 0, 0, 0, 0, {}), (what, x)
        for x in asked:                                                                    # w + d is a second witness
            d = first["directions"][x]["d"]
            if res["classes"][x] != FREE:
                continue
            assert d[x] == 1, (what, x)
            moved = base.copy()
            for t, v in d.items():
                moved[t] = np.frombuffer(((c["w"][t] + v) % R).to_bytes(32, "little"), dtype=np.uint8)
            assert set(circ.check(moved)[1].tolist()) <= set(res["broken"]), (what, x)   # no unbroken constraint breaks: 0 broken on a satisfied circuit
        return s
    finally:
        circ.close()


def directed(ctx, name, others=1):
    return assert_case(ctx, osr.DIRECTED[name], osr.result(name), name, others)


def test_two_by_two(ctx):
    assert directed(ctx, "2x2_regular")["status"].tolist() == [FIXED, FORCED, FORCED]
    assert directed(ctx, "2x2_singular")["status"].tolist() == [FIXED, FREE, FREE]          # the pivot wire's direction: an inverse
    for name in ("2x2_singular_mod_r", "2x2_singular_large_k"):                             # a remainder equal to r is zero
        assert directed(ctx, name)["status"].tolist() == [FIXED, FREE, FREE], name


def test_rank_depends_on_the_witness(ctx):
    assert directed(ctx, "selector_0")["status"].tolist() == [FIXED, FIXED, FREE, FORCED]
    assert directed(ctx, "selector_1")["status"].tolist() == [FIXED, FIXED, FREE, FREE]


def test_cross_terms(ctx):
    assert directed(ctx, "square_y_fixed")["status"].tolist() == [FIXED, UNDECIDED, FIXED]
    assert directed(ctx, "square_open")["status"].tolist() == [FIXED, UNDECIDED, UNDECIDED]
    assert directed(ctx, "product_alone")["status"].tolist() == [FIXED, UNDECIDED, UNDECIDED, UNDECIDED]
    assert directed(ctx, "product_with_sums")["status"].tolist() == [FIXED, FORCED, FORCED, UNDECIDED]


def test_audit_finishes_the_product(ctx):
    """x + y, x - y, x y = z: pass 1 forces x and y and leaves z UNDECIDED, pass 2's closure pins z"""
    import k16
    c = osr.DIRECTED["product_with_sums"]
    circ = k16.R1cs(ctx, rb.write(*c["circuit"]))
    try:
        assert circ.check(rb.witness_bytes(c["w"]))[0] == 0
        classes, forced_in, passes = circ.audit(seed=[0])
        assert (classes.tolist(), forced_in.tolist(), passes) == ([FIXED] * 4, [0, 1, 1, 0], 2)
        classes, forced_in, passes = circ.audit(seed=[0, 3], max_passes=2)                  # z given: the same two passes
        assert (classes.tolist(), forced_in.tolist(), passes) == ([FIXED] * 4, [0, 1, 1, 0], 2)
        with pytest.raises(RuntimeError):
            circ.audit(seed=[0], max_passes=1)
    finally:
        circ.close()
    circ = k16.R1cs(ctx, rb.write(*c["circuit"], n_prv_in=0))                               # the header names no input: the default seed is wire 0
    try:
        assert circ.check(rb.witness_bytes(c["w"]))[0] == 0
        classes, forced_in, passes = circ.audit()
        assert (classes.tolist(), forced_in.tolist(), passes) == ([FIXED] * 4, [0, 1, 1, 0], 2)
    finally:
        circ.close()


def test_broken_constraints(ctx):
    assert directed(ctx, "broken_anchor")["status"].tolist() == [FIXED] + [FREE] * 5
    s = directed(ctx, "only_in_broken")
    assert s["status"].tolist() == [FIXED, FREE, FREE, FREE] and s["comp"].tolist() == [osr.NO_COMP, 1, 2, 2]


def test_merged_coefficients(ctx):
    assert directed(ctx, "merged_terms")["status"].tolist() == [FIXED, ABSENT, FORCED, FORCED]


@pytest.mark.parametrize("n", osr.CHAIN_SIZES)
def test_chains(ctx, n):
    """both sides of every size class's edge; in the open 64-wire chain the free column is the last lane"""
    assert directed(ctx, "chain_%d_anchored" % n, others=8)["status"].tolist() == [FIXED] + [FORCED] * n
    s = directed(ctx, "chain_%d_open" % n)
    assert s["status"].tolist() == [FIXED] + [FREE] * n and s["n_dims"] == 1


def test_chain_of_65_is_skipped(ctx):
    for name in ("chain_65_anchored", "chain_65_open"):
        s = directed(ctx, name)
        assert s["status"].tolist() == [FIXED] + [SKIPPED] * 65 and s["n_skipped"] == 65, name


def test_redundant_and_dense_rows(ctx):
    assert directed(ctx, "redundant_rows")["status"].tolist() == [FIXED, FREE, FREE, FREE]
    assert directed(ctx, "dense_64")["n_dims"] == 61
    assert directed(ctx, "dense_64_full", others=8)["status"].tolist() == [FIXED] + [FORCED] * 64


@pytest.mark.parametrize("name", ["redundant_rows", "chain_17_open", "product_with_sums", "dense_64"])
def test_row_order(ctx, name):
    c = osr.permuted(osr.DIRECTED[name])
    res = osr.analyse(c["circuit"], c["w"], c["fixed"])
    s = assert_case(ctx, c, res, name)
    assert s["status"].tolist() == osr.result(name)["classes"]
    for x, k in enumerate(res["classes"]):                                                 # (the device's were compared with res's)
        assert osr.direction(res, x) == osr.direction(osr.result(name), x), (name, x)


def test_many_components(ctx):
    """one launch per size class over about 1,000 components"""
    c = osr.many_components()
    res = osr.analyse(c["circuit"], c["w"], c["fixed"])
    sizes = [len(k["wires"]) for k in res["comps"].values()]
    assert len(sizes) == 1000 and min(sum(n <= 16 for n in sizes), sum(16 < n <= 32 for n in sizes), sum(32 < n for n in sizes)) >= 10
    assert min(res["n_forced"], res["n_free"], res["n_undecided"]) >= 100
    assert_case(ctx, c, res, others=32)


@pytest.mark.parametrize("block", range(8))
def test_random_family(ctx, block):
    per = osr.N_RANDOM // 8
    for seed in range(block * per, block * per + per):
        assert_case(ctx, osr.random_case(seed), osr.random_result(seed), seed)


def test_fixed_as_bytes_and_cap(ctx):
    """a byte mask instead of a list; cap cuts the list, not the counts"""
    import k16
    c, res = osr.random_case(1), osr.random_result(1)
    circ = k16.R1cs(ctx, rb.write(*c["circuit"]))
    try:
        circ.check(rb.witness_bytes(c["w"]))
        mask = np.zeros(c["circuit"][0], dtype=np.uint8)
        mask[c["fixed"]] = 7
        mask[0] = 0                                                                        # wire 0 is fixed whatever the mask says
        full = circ.open_system(mask, want_maps=True)
        assert full["status"].tolist() == res["classes"]
        cut = circ.open_system(mask, cap=3)
        assert cut["wires"].tolist() == res["listed"][:3] and cut["n_free"] == res["n_free"]
    finally:
        circ.close()


def raw_system(circ, mask, cap=0, lists=False, maps=False, fill=0xAB):
    n_wires = circ.info()["n_wires"]
    counts = [C.c_uint64(fill) for _ in range(7)]
    wires, cls = np.full(max(cap, 1) + 1, fill, dtype=np.uint32), np.full(max(cap, 1) + 1, fill, dtype=np.uint8)
    status, comp = np.full(n_wires, fill, dtype=np.uint8), np.full(n_wires, fill, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = circ.ctx.L.k16_r1cs_open_system(circ.h, p(mask) if mask is not None else None, *(C.byref(x) for x in counts),
                                         p(wires) if lists else None, p(cls) if lists else None, cap, p(status) if maps else None,
                                         p(comp) if maps else None)
    return rc, [x.value for x in counts], wires, cls, status, comp


def raw_direction(circ, mask, wire, cap=64, outputs=True, fill=0xAB):
    cls, n = C.c_uint8(fill), C.c_uint64(fill)
    nums = [C.c_uint32(fill) for _ in range(4)]
    wires, vals = np.full(65, fill, dtype=np.uint32), np.full((65, 32), fill, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = circ.ctx.L.k16_r1cs_open_direction(circ.h, p(mask) if mask is not None else None, wire, C.byref(cls),
                                            *((C.byref(x) for x in nums) if outputs else [None] * 4), C.byref(n),
                                            p(wires) if outputs else None, p(vals) if outputs else None, cap)
    return rc, cls.value, [x.value for x in nums], n.value, wires, vals


def test_argument_errors(ctx):
    import k16
    c, res = osr.DIRECTED["chain_17_open"], osr.result("chain_17_open")
    circ = k16.R1cs(ctx, rb.write(*c["circuit"]))
    try:
        mask = np.zeros(18, dtype=np.uint8)
        rc, counts, wires, cls, status, comp = raw_system(circ, mask, cap=4, lists=True, maps=True)      # no completed check
        assert rc == ERR_ARG and counts == [0] * 7
        assert (wires == 0xAB).all() and (cls == 0xAB).all() and (status == 0xAB).all() and (comp == 0xAB).all()
        assert raw_direction(circ, mask, 1)[0] == ERR_ARG
        assert circ.check(rb.witness_bytes(c["w"]))[0] == 0
        assert raw_system(circ, None)[0] == ERR_ARG and raw_direction(circ, None, 1)[0] == ERR_ARG        # no mask
        rc, k, nums, n, wires, vals = raw_direction(circ, mask, 18)                                       # wire out of range
        assert (rc, n, nums) == (ERR_ARG, 0, [0] * 4) and (wires == 0xAB).all() and (vals == 0xAB).all()
        # cap = 0 and every optional output NULL: the counts alone
        rc, counts, wires, cls, status, comp = raw_system(circ, mask)
        assert rc == 0 and counts == [0, 17, 0, 0, 0, 1, 1]
        assert (wires == 0xAB).all() and (cls == 0xAB).all() and (status == 0xAB).all() and (comp == 0xAB).all()
        # the list stops at cap: nothing is written behind it
        rc, counts, wires, cls, status, comp = raw_system(circ, mask, cap=4, lists=True, maps=True)
        assert rc == 0 and wires.tolist() == [1, 2, 3, 4, 0xAB] and cls.tolist() == [FREE] * 4 + [0xAB]
        assert status.tolist() == res["classes"] and comp.tolist() == res["comp"]
        rc, k, nums, n, wires, vals = raw_direction(circ, mask, 5, outputs=False)
        assert (rc, k, n) == (0, FREE, 17)
        rc, k, nums, n, wires, vals = raw_direction(circ, mask, 5, cap=2)
        assert (rc, k, nums, n) == (0, FREE, [17, 16, 0, 16], 17)
        assert wires[:3].tolist() == [1, 2, 0xAB] and (vals[2:] == 0xAB).all()
        assert [int.from_bytes(vals[i].tobytes(), "little") for i in range(2)] == [1, R - 1]
        # after an error the object still answers
        assert raw_direction(circ, mask, 99)[0] == ERR_ARG
        assert circ.open_system([0])["n_free"] == 17
    finally:
        circ.close()
