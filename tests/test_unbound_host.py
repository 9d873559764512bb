"""CPU tests of the unbound-wire scan's host side: keyless-zk-proofs_amd/csrc/r1cs_pairs.h, the (wire, constraint) incidence
list, through tests/cpp/r1cs_pairs_check.cpp -- a stand-alone program built with -fsanitize=address,undefined and run as a plain
subprocess -- against the merged incidences of tests/unbound_reference.py; and the reference itself on the directed circuits,
whose classes are known by construction."""
import os
import subprocess

import pytest

import r1cs_builder as rb
import unbound_reference as ur
from unbound_reference import ABSENT, BOUND, UNBOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("unbound_host") / "r1cs_pairs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_pairs_check.cpp"), "-o", out], timeout=600)
    return out


def expected(n_wires, rowsA, rowsB, rowsC):
    inc = ur.incidences(n_wires, rowsA, rowsB, rowsC)
    present = sorted({s for s, _, _, _, _ in inc})
    return inc, present


def listed(exe, tmp_path, circuits):
    """The program's output for a list of circuits, one file each, in one run: [(incidences, side, present)]"""
    paths = []
    for i, circ in enumerate(circuits):
        p = tmp_path / ("c%d.r1cs" % i)
        p.write_bytes(rb.write(*circ[:4]))
        paths.append(str(p))
    out = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]     # the sanitizers stay silent
    lines, res = out.stdout.splitlines(), []
    at = 0
    for circ in circuits:
        assert lines[at] == "rc=0", lines[at]
        head = dict(x.split("=") for x in lines[at + 1].split())
        n = int(head["pairs"])
        assert int(head["wires"]) == circ[0]
        inc = [(int(f[0]), int(f[1]), int(f[2], 16), int(f[3], 16), int(f[4], 16)) for f in (l.split() for l in lines[at + 2:at + 2 + n])]
        assert lines[at + 2 + n].startswith("present=")
        res.append((inc, int(head["side"]), [int(x) for x in lines[at + 2 + n][8:].split()]))
        at += 3 + n
    assert at == len(lines)
    return res


def test_directed_circuits_list_the_references_incidences(exe, tmp_path):
    names = sorted(ur.DIRECTED)
    got = listed(exe, tmp_path, [ur.DIRECTED[n] for n in names])
    for name, (inc, side, present) in zip(names, got):
        want_inc, want_present = expected(*ur.DIRECTED[name][:4])
        assert inc == want_inc and present == want_present, name
    by_name = dict(zip(names, got))
    assert by_name["cancellation_alone"][1] == 0                    # a sum of zero takes no place in the side table
    # the block edges: what the scan WALKS -- the incidences of the wires from 1 on -- numbers exactly 255, 256, 257
    walked = lambda inc: sum(1 for s, _, _, _, _ in inc if s != 0)
    assert [walked(by_name["pairs_%d_%s" % (t, k)][0]) for t in (255, 256, 257) for k in ("free", "bound")] == [255, 255, 256, 256, 257, 257]


def test_random_circuits_list_the_references_incidences(exe, tmp_path):
    circuits = [ur.random_circuit(seed) for seed in range(ur.N_RANDOM)]
    got = listed(exe, tmp_path, circuits)
    sides = 0
    for seed, (circ, (inc, side, present)) in enumerate(zip(circuits, got)):
        want_inc, want_present = expected(*circ[:4])
        assert inc == want_inc and present == want_present, seed
        sides += side
    assert sides > 40                                               # wires listed twice whose sum is not zero: the side table is in use


def classes_of(name):
    return ur.classify(*ur.DIRECTED[name])


def test_reference_classifies_the_directed_circuits_as_constructed():
    # mux: sel (x - y) = out - y over wires 1 sel, 2 x, 3 y, 4 out
    assert classes_of("mux_sel0") == [BOUND, BOUND, UNBOUND, BOUND, BOUND]
    assert classes_of("mux_sel1")[2] == BOUND
    assert classes_of("square_at_zero") == [BOUND, BOUND, BOUND]              # lin = 0, quad = 1
    for name in ur.DIRECTED:
        if name.startswith("tautology"):
            assert classes_of(name) == [BOUND, UNBOUND], name                 # for every k and every x: not ABSENT
    assert classes_of("cancellation_alone")[2] == ABSENT
    assert classes_of("cancellation_elsewhere")[2] == BOUND
    n_wires, rowsA, rowsB, rowsC, w = ur.DIRECTED["zero_only_modulo_r"]
    lin = rowsA[0][0][1] * rb.dot(rowsB[0], w) - rowsC[0][0][1]
    assert lin != 0 and lin % ur.R == 0                                       # zero only modulo r ...
    assert classes_of("zero_only_modulo_r") == [BOUND, UNBOUND]
    for n, at in ur.COLUMN_CASES:
        assert classes_of("column_%d_%s" % (n, at))[1] == (UNBOUND if at is None else BOUND), (n, at)
        assert len(ur.wire_constraints(*ur.DIRECTED["column_%d_%s" % (n, at)][:4], 1)) == n
    for n in (64, 65, 128, 129):
        cl = classes_of("wires_%d" % n)
        assert [s for s, k in enumerate(cl) if k != BOUND] == [s for s in (63, 64, 127, 128) if s < n]
        assert all(cl[s] == UNBOUND for s in (63, 64, 127, 128) if s < n)
    for t in (255, 256, 257):
        assert classes_of("pairs_%d_bound" % t)[-1] == BOUND and classes_of("pairs_%d_free" % t)[-1] == UNBOUND
        for k in ("bound", "free"):
            circ = ur.DIRECTED["pairs_%d_%s" % (t, k)][:4]
            inc = ur.incidences(*circ)
            assert len(inc) - len(ur.wire_constraints(*circ, 0)) == t         # walked: all but wire 0's column
            assert inc[-1][0] == circ[0] - 1                                  # the last incidence is the highest wire's
            cl = classes_of("pairs_%d_%s" % (t, k))[1:2 * ((t - 1) // 2) + 1]
            assert cl.count(BOUND) == cl.count(UNBOUND) == (t - 1) // 2       # bound and free wires alternate up to it
    cl = classes_of("unused_wires")
    assert cl[3] == ABSENT and cl[5] == ABSENT and cl.count(ABSENT) == 2
    for name, circ in ur.DIRECTED.items():
        assert rb.check(*circ[1:]) == [], name                                # every directed witness satisfies its circuit


def test_every_random_circuit_holds_all_three_classes_and_its_plants():
    for seed in range(ur.N_RANDOM):
        n_wires, rowsA, rowsB, rowsC, w, w_broken, (absent, taut, mux_x) = ur.random_circuit(seed)
        assert rb.check(rowsA, rowsB, rowsC, w) == [] and rb.check(rowsA, rowsB, rowsC, w_broken), seed
        for ww in (w, w_broken):
            cl = ur.classify(n_wires, rowsA, rowsB, rowsC, ww)
            assert (cl[absent], cl[taut], cl[mux_x]) == (ABSENT, UNBOUND, UNBOUND), seed
            assert cl.count(BOUND) > 1, seed                                  # (wire 0 is BOUND by definition: one more)
