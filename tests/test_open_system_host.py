"""CPU tests of the open-set solve's host side and of its reference (include/k16.h k16_r1cs_open_system / _open_direction,
DESIGN.md section 10h): tests/open_system_reference.py against brute force over F_7 and on circuits whose answer is stated by
hand, the condition on the random family the GPU test shares, and keyless-zk-proofs_amd/csrc/r1cs_open.h -- kinds, components,
work list -- through tests/cpp/r1cs_open_check.cpp, a stand-alone program built with -fsanitize=address,undefined and run as a
plain subprocess."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import open_system_reference as osr
import r1cs_builder as rb
from open_system_reference import ABSENT, FIXED, FORCED, FREE, SKIPPED, UNDECIDED, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_symbols():
    import k16
    assert (k16.OPEN_FIXED, k16.OPEN_ABSENT, k16.OPEN_FORCED, k16.OPEN_FREE, k16.OPEN_UNDECIDED, k16.OPEN_SKIPPED) == \
        (FIXED, ABSENT, FORCED, FREE, UNDECIDED, SKIPPED) == (0, 1, 2, 3, 4, 5)
    assert k16.OPEN_MAX_WIRES == osr.MAX_WIRES == 64 and k16.OPEN_NO_COMPONENT == osr.NO_COMP
    hdr = open(os.path.join(ROOT, "include", "k16.h")).read()
    for s in ("k16_r1cs_open_system", "k16_r1cs_open_direction"):
        assert s in k16.SYMBOLS and "int  %s(" % s in hdr
    assert "#define K16_OPEN_MAX_WIRES 64" in hdr
    assert "K16_OPEN_FIXED = 0, K16_OPEN_ABSENT = 1, K16_OPEN_FORCED = 2, K16_OPEN_FREE = 3, K16_OPEN_UNDECIDED = 4, K16_OPEN_SKIPPED = 5" in hdr
    for m in ("open_system", "open_direction", "audit"):
        assert callable(getattr(k16.R1cs, m))


# ---------------------------------------------------------------- brute force over F_7
def solutions(circuit, w, fixed, p):
    """every assignment of the outside wires that keeps the constraints w satisfies satisfied: rows of an array"""
    n_wires, rowsA, rowsB, rowsC = circuit
    keep = [i for i in range(len(rowsA)) if i not in osr.broken(circuit, w, p)]
    outside = [s for s in range(1, n_wires) if s not in fixed]
    grid = np.array(list(itertools.product(range(p), repeat=len(outside))), dtype=np.int64).reshape(p ** len(outside), len(outside))
    W = np.tile(np.array(w, dtype=np.int64), (grid.shape[0], 1))
    W[:, outside] = grid

    def vec(row):
        v = np.zeros(n_wires, dtype=np.int64)
        for s, k in row:
            v[s] += k
        return v % p

    ok = np.ones(W.shape[0], dtype=bool)
    for i in keep:
        ok &= (W @ vec(rowsA[i]) % p) * (W @ vec(rowsB[i]) % p) % p == W @ vec(rowsC[i]) % p
    return W[ok]


def test_reference_against_brute_force():
    """3,000 random circuits of 3 .. 6 wires over F_7, every assignment of the outside wires enumerated: no FORCED wire takes a
    second value, every FREE wire does, and w + d of every FREE wire is a solution"""
    p, seen = 7, {FORCED: 0, FREE: 0, UNDECIDED: 0}
    for seed in range(3000):
        circuit, w, fixed = osr.small_random(seed, p)
        res = osr.analyse(circuit, w, fixed, p)
        sol = solutions(circuit, w, set(fixed) | {0}, p)
        assert sol.shape[0] >= 1
        before = set(osr.broken(circuit, w, p))
        for s, k in enumerate(res["classes"]):
            if k in seen:
                seen[k] += 1
            varies = bool((sol[:, s] != w[s]).any())
            if k == FORCED:
                assert not varies, (seed, s)
            elif k == FREE:
                assert varies, (seed, s)
                d = osr.direction(res, s)
                assert d[s] == 1 and all(res["comp"][t] == res["comp"][s] for t in d), (seed, s)
                assert set(osr.broken(circuit, osr.moved(w, d, p), p)) <= before, (seed, s)
            else:
                assert osr.direction(res, s) == {}
    assert min(seen.values()) > 300, seen


# ---------------------------------------------------------------- directed circuits: what each must give
def classes_of(name):
    return osr.result(name)["classes"]


def test_directed_two_by_two():
    assert classes_of("2x2_regular") == [FIXED, FORCED, FORCED]
    for name in ("2x2_singular", "2x2_singular_mod_r", "2x2_singular_large_k"):
        res = osr.result(name)
        assert res["classes"] == [FIXED, FREE, FREE] and res["comps"][1]["rank"] == 1 and res["n_dims"] == 1, name
    res = osr.result("2x2_singular")                               # x + 2 y: moving y by 1 moves x by -2; x by 1, y by -1/2
    assert osr.direction(res, 2) == {1: R - 2, 2: 1}
    assert osr.direction(res, 1) == {1: 1, 2: (R - pow(2, R - 2, R)) % R}


def test_directed_rank_depends_on_the_witness():
    res = osr.result("selector_0")                                 # s = 0: x is free alone, y is forced
    assert res["classes"] == [FIXED, FIXED, FREE, FORCED] and osr.direction(res, 2) == {2: 1}
    res = osr.result("selector_1")                                 # s = 1: x and y move together
    assert res["classes"] == [FIXED, FIXED, FREE, FREE] and osr.direction(res, 2) == {2: 1, 3: 1} == osr.direction(res, 3)


def test_directed_cross_terms():
    assert classes_of("square_y_fixed") == [FIXED, UNDECIDED, FIXED]
    assert classes_of("square_open") == [FIXED, UNDECIDED, UNDECIDED]
    assert classes_of("product_alone") == [FIXED, UNDECIDED, UNDECIDED, UNDECIDED]
    res = osr.result("product_with_sums")
    assert res["classes"] == [FIXED, FORCED, FORCED, UNDECIDED] and res["n_dims"] == 0 and res["n_components"] == 1
    assert res["kinds"] == [osr.KIND_CROSS, osr.KIND_LINEAR, osr.KIND_LINEAR]


def test_directed_broken_constraints():
    res = osr.result("broken_anchor")
    assert res["classes"] == [FIXED] + [FREE] * 5 and res["comps"][1]["rank"] == 4
    res = osr.result("only_in_broken")
    assert res["classes"] == [FIXED, FREE, FREE, FREE] and res["comp"][1:] == [1, 2, 2]
    assert res["comps"][1]["rank"] == 0 and res["comps"][1]["rows"] == [] and osr.direction(res, 1) == {1: 1}


def test_directed_merged_coefficients():
    res = osr.result("merged_terms")                               # wire 1 cancels: ABSENT; wire 2 forced by row 0, then wire 3
    assert res["classes"] == [FIXED, ABSENT, FORCED, FORCED]
    assert res["lin_rows"][0] == {2: 3} and res["lin_rows"][1] == {2: 1, 3: 5}


@pytest.mark.parametrize("n", osr.CHAIN_SIZES)
def test_directed_chains(n):
    assert classes_of("chain_%d_anchored" % n) == [FIXED] + [FORCED] * n
    res = osr.result("chain_%d_open" % n)
    assert res["classes"] == [FIXED] + [FREE] * n and res["comps"][1]["rank"] == n - 1 and res["n_dims"] == 1
    for x in (1, n // 2, n):
        d = osr.direction(res, x)
        assert d == {s: 1 if (s - x) % 2 == 0 else R - 1 for s in range(1, n + 1)}


def test_directed_skipped_and_redundant():
    for name in ("chain_65_anchored", "chain_65_open"):
        res = osr.result(name)
        assert res["classes"] == [FIXED] + [SKIPPED] * 65 and res["n_skipped"] == 65 and res["n_components"] == 1
    res = osr.result("redundant_rows")
    assert res["comps"][1]["rank"] == 2 and len(res["comps"][1]["rows"]) == 12 and res["classes"] == [FIXED, FREE, FREE, FREE]
    assert osr.result("dense_64")["comps"][1]["rank"] == 3 and osr.result("dense_64_full")["classes"] == [FIXED] + [FORCED] * 64


def test_directed_row_order():
    for name in ("redundant_rows", "chain_17_open", "product_with_sums", "dense_64"):
        c = osr.DIRECTED[name]
        a, b = osr.result(name), osr.analyse(**{k: v for k, v in osr.permuted(c).items()})
        assert a["classes"] == b["classes"] and a["comp"] == b["comp"], name
        for s, k in enumerate(a["classes"]):
            assert osr.direction(a, s) == osr.direction(b, s), (name, s)


def test_directions_move_to_another_witness():
    for name, c in sorted(osr.DIRECTED.items()):
        res = osr.result(name)
        before = set(osr.broken(c["circuit"], c["w"]))
        for s in [s for s, k in enumerate(res["classes"]) if k == FREE][:6]:
            d = osr.direction(res, s)
            assert d[s] == 1 and set(osr.broken(c["circuit"], osr.moved(c["w"], d))) <= before, (name, s)


def test_random_family_condition():
    """what the family the GPU test shares must hold, from the reference alone"""
    count = {FORCED: 0, FREE: 0, UNDECIDED: 0}
    rich, mid, large = 0, 0, 0
    for seed in range(osr.N_RANDOM):
        res = osr.random_result(seed)
        for k in count:
            count[k] += res["classes"].count(k)
        for comp in res["comps"].values():
            n = len(comp["wires"])
            mid += 17 <= n <= 32
            large += 33 <= n <= 64
            rich += (not comp["skipped"]) and comp["exact"] and comp["rank"] >= 2 and n - comp["rank"] >= 1
    assert min(count.values()) >= 10, count
    assert rich >= 5 and mid >= 1 and large >= 1, (rich, mid, large)


# ---------------------------------------------------------------- r1cs_open.h
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("open_host") / "r1cs_open_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_open_check.cpp"), "-o", out], timeout=600)
    return out


def run(exe, path, c, res, wire=None):
    args = [exe, path, ",".join(map(str, c["fixed"])) or "-", ",".join(map(str, res["broken"])) or "-"]
    out = subprocess.run(args + ([str(wire)] if wire is not None else []), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr and "FAIL" not in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def parse_components(lines):
    """[(id, cross, wires, [(constraint, [(column, wire)])])] in the program's order"""
    comps = []
    for ln in lines:
        f = ln.split()
        if f[0] == "component":
            comps.append((int(f[1]), int(f[2].split("=")[1]), [int(x) for x in f[3].split("=")[1].split(",")], []))
        elif f[0] == "row":
            comps[-1][3].append((int(f[1]), [tuple(int(x) for x in e.split(":")) for e in f[2:]]))
    return comps


def expected_component(res, cid):
    k = res["comps"][cid]
    rows = [(i, [(k["wires"].index(s), s) for s in sorted(res["lin_rows"][i])]) for i in k["rows"]]
    return (cid, k["cross"], k["wires"], rows)


HOST_CASES = ["product_with_sums", "only_in_broken", "merged_terms", "selector_0", "broken_anchor", "chain_17_open", "chain_65_open",
              "redundant_rows", "square_y_fixed"]


def test_host_program(exe, tmp_path):
    cases = [(name, osr.DIRECTED[name], osr.result(name)) for name in HOST_CASES]
    cases += [("random_%d" % s, osr.random_case(s), osr.random_result(s)) for s in (0, 1, 5)]
    for name, c, res in cases:
        path = str(tmp_path / (name + ".r1cs"))
        with open(path, "wb") as f:
            f.write(rb.write(*c["circuit"]))
        lines = run(exe, path, c, res)
        assert lines[0] == "kinds " + "".join(map(str, res["kinds"])), name
        sizes = [len(k["wires"]) for k in res["comps"].values() if not k["skipped"]]
        want = "counts components=%d skipped=%d absent=%d classes=%d,%d,%d" % (
            res["n_components"], res["n_skipped"], res["n_absent"], sum(n <= 16 for n in sizes), sum(16 < n <= 32 for n in sizes),
            sum(32 < n for n in sizes))
        assert lines[1] == want, name
        host_cls = {FIXED: 0, ABSENT: 1, SKIPPED: 5}
        assert lines[2] == "cls " + "".join(str(host_cls.get(k, 2)) for k in res["classes"]), name
        assert lines[3] == "comp " + " ".join("-" if k == osr.NO_COMP else str(k) for k in res["comp"]), name
        live = sorted((cid for cid, k in res["comps"].items() if not k["skipped"]),
                      key=lambda cid: (len(res["comps"][cid]["wires"]) > 16, len(res["comps"][cid]["wires"]) > 32, cid))
        assert parse_components(lines[4:]) == [expected_component(res, cid) for cid in live], name
        # the walk from one wire finds the same component
        for wire in sorted({0, 1, len(res["classes"]) - 1} | set(c["fixed"][:1])):
            one = run(exe, path, c, res, wire)
            k = res["classes"][wire]
            comp = res["comps"].get(res["comp"][wire])
            if k in (FIXED, ABSENT):
                assert one[0] == "one class=%d wires=0 rows=0 cross=0" % k, (name, wire)
                continue
            assert one[0] == "one class=%d wires=%d rows=%d cross=%d" % (
                5 if comp["skipped"] else 2, len(comp["wires"]), len(comp["rows"]), comp["cross"]), (name, wire)
            assert parse_components(one[1:]) == ([] if comp["skipped"] else [expected_component(res, res["comp"][wire])]), (name, wire)
