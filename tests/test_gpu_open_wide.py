"""-m gpu : the wide classes of the open-set solve (include/k16.h k16_r1cs_open_system_ex / k16_r1cs_open_direction_ex;
csrc/r1cs_scan.hip k_r1cs_open_rref_wide, csrc/r1cs_open.h) against the big-integer reference of
tests/open_system_reference.py, which takes the cap.  Every case compares the counts, the list, the class and the component of
every wire, and the component's sizes, the rank and the direction of the wires it asks about, byte for byte with the
reference; every case runs twice for equal bytes; and for each FREE wire asked about the direction is added to the witness
and the check must find no constraint broken that it did not find broken before.  Directions are asked for the 8 lowest and
the 8 highest FREE wires of a component (all of them where it has at most 16) and for the first and the last wire of the other
classes; the second run repeats every one of them.  Two cases ask less, for time: test_all_five_classes (200 components) and
test_more_components_than_slabs (68) ask 8 + 8 of some components -- the first two with a FREE wire of each size, and in the
second case the four whose slab is reused as well -- and the lowest and highest FREE wire of every other one; with 8 + 8
everywhere they take 17.6 s and 13.9 s on an MI355X, each direction call eliminating its component again.  What each circuit's classes must be is asserted of the reference itself in tests/test_open_wide_host.py."""
import ctypes as C

import numpy as np
import pytest

import open_system_reference as osr
import open_wide_reference as owr
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


def asked_wires(res, full=None):
    """full: None, or the ids of the components whose 8 lowest and 8 highest FREE wires are asked; the others give their lowest
    and their highest FREE wire"""
    asked = set()
    for cid, k in res["comps"].items():
        free = [s for s in k["wires"] if res["classes"][s] == FREE]
        per = 8 if full is None or cid in full else 1
        asked |= set(free if len(free) <= 2 * per else free[:per] + free[-per:])
    rest = [x for x in res["listed"] if res["classes"][x] != FREE]
    return sorted(asked | set(rest[:1] + rest[-1:]))


def snapshot(circ, c, asked, max_wires):
    """everything both calls report, in a form that compares byte for byte"""
    s = circ.open_system(c["fixed"], want_maps=True, max_wires=max_wires)
    out = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    out["directions"] = {x: circ.open_direction(c["fixed"], x, max_wires=max_wires) for x in asked}
    return s, out


def assert_case(ctx, c, res, what=None, max_wires=256, full=None):
    """check, both calls twice, against the reference (built with the same cap); then the FREE directions through the check"""
    import k16
    n_wires, rowsA, rowsB, rowsC = c["circuit"]
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        base = rb.witness_bytes(c["w"])
        n_failed, failed = circ.check(base)
        assert failed.tolist() == res["broken"], what
        asked = asked_wires(res, full)
        s, first = snapshot(circ, c, asked, max_wires)
        again = asked                                                                      # the second run: every map, every asked direction
        s2, second = snapshot(circ, c, again, max_wires)
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
        moved_any = False
        for x in asked:                                                                    # w + d is a second witness
            d = first["directions"][x]["d"]
            if res["classes"][x] != FREE:
                continue
            assert d[x] == 1, (what, x)
            moved = base.copy()
            for t, v in d.items():
                moved[t] = np.frombuffer(((c["w"][t] + v) % R).to_bytes(32, "little"), dtype=np.uint8)
            assert set(circ.check(moved)[1].tolist()) <= set(res["broken"]), (what, x)   # no constraint breaks that was not broken
            moved_any = True
        if moved_any:
            circ.check(base)
        return s
    finally:
        circ.close()


def full_of(res, per_size=2):
    """the first per_size components with a FREE wire of each number of wires"""
    seen, full = {}, set()
    for cid in sorted(res["comps"]):
        k = res["comps"][cid]
        if any(res["classes"][s] == FREE for s in k["wires"]) and seen.setdefault(len(k["wires"]), 0) < per_size:
            seen[len(k["wires"])] += 1
            full.add(cid)
    return full


def named(ctx, name, max_wires=256, full=None):
    return assert_case(ctx, owr.circuit(name), owr.result(name, max_wires), name, max_wires, full)


@pytest.mark.parametrize("n", owr.CHAIN_SIZES)
def test_chains(ctx, n):
    """both sides of both wide classes' edges; in the open chain the free column is the last thread of the last wave"""
    assert named(ctx, "chain_%d_anchored" % n)["status"].tolist() == [FIXED] + [FORCED] * n
    s = named(ctx, "chain_%d_open" % n)
    assert s["status"].tolist() == [FIXED] + [FREE] * n and s["n_dims"] == 1


def test_chains_above_the_cap(ctx):
    s = named(ctx, "chain_257_open")
    assert s["status"].tolist() == [FIXED] + [SKIPPED] * 257 and s["n_skipped"] == 257
    assert named(ctx, "chain_257_anchored")["n_skipped"] == 257
    assert named(ctx, "chain_129_open", max_wires=128)["status"].tolist() == [FIXED] + [SKIPPED] * 129
    assert named(ctx, "chain_129_open", max_wires=256)["status"].tolist() == [FIXED] + [FREE] * 129
    assert named(ctx, "chain_129_anchored", max_wires=200)["n_forced"] == 129


def test_chain_of_65_at_cap_64_is_the_unchanged_call(ctx):
    import k16
    for name in ("chain_65_open", "chain_65_anchored"):
        c = owr.circuit(name)
        assert named(ctx, name, max_wires=64)["status"].tolist() == [FIXED] + [SKIPPED] * 65
        circ = k16.R1cs(ctx, rb.write(*c["circuit"]))
        try:
            assert circ.check(rb.witness_bytes(c["w"]))[0] == 0
            a, b = circ.open_system([0], want_maps=True), circ.open_system([0], want_maps=True, max_wires=64)
            assert {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in a.items()} == \
                {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
            assert circ.open_direction([0], 7) == circ.open_direction([0], 7, max_wires=64)
        finally:
            circ.close()


@pytest.mark.parametrize("name", sorted(owr.DENSE))
def test_dense_rows(ctx, name):
    n, n_rows, _ = owr.DENSE[name]
    s = named(ctx, name)
    assert s["n_dims"] == max(0, n - n_rows) and s["n_forced"] == (n if n_rows >= n else 0)


def test_redundant_rows(ctx):
    """12 rows of rank 2 over 100 wires: ten remainders are zero only mod r"""
    s = named(ctx, "redundant_100")
    assert s["status"].tolist() == [FIXED] + [FREE] * 100 and s["n_dims"] == 98


def test_cross_in_a_wide_component(ctx):
    """an anchored chain of 100 wires and x_1 x_2 = x_101: FORCED comes from the LINEAR rows of a component that is not EXACT,
    and the audit with the wide cap finishes what the audit without it cannot start"""
    import k16
    s = named(ctx, "cross_chain")
    assert s["status"].tolist() == [FIXED] + [FORCED] * 100 + [UNDECIDED]
    c = owr.circuit("cross_chain")
    circ = k16.R1cs(ctx, rb.write(*c["circuit"], n_prv_in=0))
    try:
        assert circ.check(rb.witness_bytes(c["w"]))[0] == 0
        classes, forced_in, passes = circ.audit(max_wires=256)
        assert (classes.tolist(), forced_in.tolist(), passes) == ([FIXED] * 102, [0] + [1] * 100 + [0], 2)
        classes, forced_in, passes = circ.audit()
        assert (classes.tolist(), forced_in.tolist(), passes) == ([FIXED] + [SKIPPED] * 101, [0] * 102, 1)
    finally:
        circ.close()


def test_broken_anchoring_row(ctx):
    s = named(ctx, "chain_130_broken")
    assert s["status"].tolist() == [FIXED] + [FREE] * 130 and s["n_dims"] == 1


@pytest.mark.parametrize("name", ["chain_129_open", "redundant_100", "cross_chain", "dense_256_40"])
def test_row_order(ctx, name):
    c = osr.permuted(owr.circuit(name))
    res = osr.analyse(c["circuit"], c["w"], c["fixed"], max_wires=256)
    s = assert_case(ctx, c, res, name)
    assert s["status"].tolist() == owr.result(name)["classes"]
    for x in asked_wires(res):                                                            # (the device's were compared with res's)
        assert osr.direction(res, x) == osr.direction(owr.result(name), x), (name, x)


def test_all_five_classes(ctx):
    """components of 3, 20, 50, 100 and 250 wires, 40 of each, in one call: five launches; the wires of the components of at
    most 64 wires get the classes of the unchanged call"""
    import k16
    c, res = owr.circuit("five_classes"), owr.result("five_classes")
    sizes = [len(k["wires"]) for k in res["comps"].values()]
    assert sorted(set(sizes)) == list(owr.FIVE_SIZES) and all(sizes.count(n) == 40 for n in owr.FIVE_SIZES)
    assert min(res["n_forced"], res["n_free"], res["n_undecided"]) >= 100
    s = assert_case(ctx, c, res, "five_classes", full=full_of(res))
    circ = k16.R1cs(ctx, rb.write(*c["circuit"]))
    try:
        assert circ.check(rb.witness_bytes(c["w"]))[0] == 0
        plain = circ.open_system(c["fixed"], want_maps=True)
        narrow = np.array([k != osr.NO_COMP and len(res["comps"][k]["wires"]) <= 64 for k in res["comp"]])
        assert narrow.sum() == 40 * 73 and (plain["status"][narrow] == s["status"][narrow]).all()
        assert (plain["status"][~narrow & (s["comp"] != osr.NO_COMP)] == SKIPPED).all() and plain["n_skipped"] == 40 * 350
        assert plain["comp"].tolist() == s["comp"].tolist()
    finally:
        circ.close()


def test_more_components_than_slabs(ctx):
    """68 components of the 256-wire class on 64 slabs: a workgroup strides to a second component, whose rank is smaller than
    the first's, on a slab nothing zeroed"""
    res = owr.result("more_than_slabs")
    comps = [res["comps"][k] for k in sorted(res["comps"])]
    assert len(comps) == owr.ARENA_SLABS_256 + 4 and all(129 <= len(k["wires"]) <= 256 for k in comps)
    for i in range(4):
        assert comps[i]["rank"] == 200 and comps[owr.ARENA_SLABS_256 + i]["rank"] == 129
    named(ctx, "more_than_slabs", full=full_of(res) | set(sorted(res["comps"])[-4:]))


@pytest.mark.parametrize("block", range(4))
def test_wide_random_family(ctx, block):
    per = owr.N_WIDE_RANDOM // 4
    for seed in range(block * per, block * per + per):
        assert_case(ctx, owr.wide_random_case(seed), owr.wide_random_result(seed), seed)


def test_directed_cases_at_cap_64(ctx):
    """every directed circuit of the 64-wire calls through the _ex calls with max_wires = 64: the bytes of the unchanged calls"""
    import k16
    for name, c in sorted(osr.DIRECTED.items()):
        res = osr.result(name)
        circ = k16.R1cs(ctx, rb.write(*c["circuit"]))
        try:
            circ.check(rb.witness_bytes(c["w"]))
            a, b = circ.open_system(c["fixed"], want_maps=True), circ.open_system(c["fixed"], want_maps=True, max_wires=64)
            assert {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in a.items()} == \
                {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in b.items()}, name
            assert a["status"].tolist() == res["classes"], name
            listed = res["listed"]
            for x in sorted(set([0] + (listed if len(listed) <= 8 else listed[:4] + listed[-4:]))):
                assert circ.open_direction(c["fixed"], x) == circ.open_direction(c["fixed"], x, max_wires=64), (name, x)
        finally:
            circ.close()


def raw_system(circ, mask, max_wires, cap=0, lists=False, maps=False, fill=0xAB):
    n_wires = circ.info()["n_wires"]
    counts = [C.c_uint64(fill) for _ in range(7)]
    wires, cls = np.full(max(cap, 1) + 1, fill, dtype=np.uint32), np.full(max(cap, 1) + 1, fill, dtype=np.uint8)
    status, comp = np.full(n_wires, fill, dtype=np.uint8), np.full(n_wires, fill, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = circ.ctx.L.k16_r1cs_open_system_ex(circ.h, p(mask) if mask is not None else None, max_wires, *(C.byref(x) for x in counts),
                                            p(wires) if lists else None, p(cls) if lists else None, cap, p(status) if maps else None,
                                            p(comp) if maps else None)
    return rc, [x.value for x in counts], wires, cls, status, comp


def raw_direction(circ, mask, max_wires, wire, cap=256, fill=0xAB):
    cls, n = C.c_uint8(fill), C.c_uint64(fill)
    nums = [C.c_uint32(fill) for _ in range(4)]
    wires, vals = np.full(257, fill, dtype=np.uint32), np.full((257, 32), fill, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = circ.ctx.L.k16_r1cs_open_direction_ex(circ.h, p(mask) if mask is not None else None, max_wires, wire, C.byref(cls),
                                               *(C.byref(x) for x in nums), C.byref(n), p(wires), p(vals), cap)
    return rc, cls.value, [x.value for x in nums], n.value, wires, vals


def test_argument_errors(ctx):
    import k16
    c, res = owr.circuit("chain_129_open"), owr.result("chain_129_open")
    circ = k16.R1cs(ctx, rb.write(*c["circuit"]))
    try:
        mask = np.zeros(130, dtype=np.uint8)
        assert raw_system(circ, mask, 256)[0] == ERR_ARG and raw_direction(circ, mask, 256, 1)[0] == ERR_ARG      # no completed check
        assert circ.check(rb.witness_bytes(c["w"]))[0] == 0
        for bad in (0, 63, 257, 2 ** 32 - 1):                              # the cap is refused before anything is written
            rc, counts, wires, cls, status, comp = raw_system(circ, mask, bad, cap=4, lists=True, maps=True)
            assert rc == ERR_ARG and counts == [0xAB] * 7, bad
            assert (wires == 0xAB).all() and (cls == 0xAB).all() and (status == 0xAB).all() and (comp == 0xAB).all(), bad
            rc, k, nums, n, wires, vals = raw_direction(circ, mask, bad, 1)
            assert (rc, k, nums, n) == (ERR_ARG, 0xAB, [0xAB] * 4, 0xAB) and (wires == 0xAB).all() and (vals == 0xAB).all(), bad
            with pytest.raises(Exception):
                circ.open_system([0], max_wires=bad)
        assert circ.open_system([0], max_wires=256)["n_free"] == 129       # the object still answers, and kept its check
        assert raw_system(circ, None, 256)[0] == ERR_ARG and raw_direction(circ, None, 256, 1)[0] == ERR_ARG      # no mask
        rc, k, nums, n, wires, vals = raw_direction(circ, mask, 256, 130)                                 # wire out of range
        assert (rc, n, nums) == (ERR_ARG, 0, [0] * 4) and (wires == 0xAB).all() and (vals == 0xAB).all()
        # cap = 0 and every optional output NULL: the counts alone
        rc, counts, wires, cls, status, comp = raw_system(circ, mask, 256)
        assert rc == 0 and counts == [0, 129, 0, 0, 0, 1, 1]
        assert (wires == 0xAB).all() and (cls == 0xAB).all() and (status == 0xAB).all() and (comp == 0xAB).all()
        rc, counts, wires, cls, status, comp = raw_system(circ, mask, 128, cap=4, lists=True, maps=True)
        assert rc == 0 and counts == [0, 0, 0, 129, 0, 1, 0] and wires.tolist() == [1, 2, 3, 4, 0xAB] and cls.tolist() == [SKIPPED] * 4 + [0xAB]
        # a direction cap below the non-zeros: the lowest cap of them, and the full count
        rc, k, nums, n, wires, vals = raw_direction(circ, mask, 256, 70, cap=3)
        assert (rc, k, nums, n) == (0, FREE, [129, 128, 0, 128], 129)
        assert wires[:4].tolist() == [1, 2, 3, 0xAB] and (vals[3:] == 0xAB).all()
        want = osr.direction(res, 70)
        assert [int.from_bytes(vals[i].tobytes(), "little") for i in range(3)] == [want[1], want[2], want[3]]
        rc, k, nums, n, wires, vals = raw_direction(circ, mask, 256, 70)
        assert n == 129 and wires[:130].tolist() == list(range(1, 130)) + [0xAB]
        rc, k, nums, n, wires, vals = raw_direction(circ, mask, 128, 70)                                  # SKIPPED under the lower cap
        assert (rc, k, nums, n) == (0, SKIPPED, [129, 128, 0, 0], 0) and (wires == 0xAB).all()
        assert raw_direction(circ, mask, 256, 999)[0] == ERR_ARG
        assert circ.open_system([0])["n_skipped"] == 129 and circ.open_system([0], max_wires=256)["n_free"] == 129
    finally:
        circ.close()
