"""CPU tests of keyless-zk-proofs_amd/csrc/setup_plan.h -- the host side of the set-up from a trapdoor (k16_r1cs_setup*):
the exact size of the key, the transposed column plan and the writer of the container, the header's integers and sections
1, 4 and 10 -- through tests/cpp/setup_plan_check.cpp, a stand-alone program built with -fsanitize=address,undefined and run
as a plain subprocess, against the Python model of tests/setup_reference.py.  The one pin that is not of our own making:
section 4 of the toy circuit's key must be byte-equal to that of the reference-made tests/golden/toy/toy_1.zkey."""
import os
import struct
import subprocess

import pytest

import r1cs_builder as rb
import setup_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("setup_host") / "setup_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "setup_plan_check.cpp"), "-o", out], timeout=600)
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]     # the sanitizers stay silent
    return out.stdout.splitlines()


def write(circuit):
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
    return rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=n_pub_out, n_pub_in=n_pub_in)


CIRCUITS = dict([("toy", sr.TOY)] + [("mixed_%d_%d_%d" % sh, sr.mixed(*sh)[0]) for sh in sr.MIXED_SHAPES])


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_size_frame_and_section_4_are_the_models(exe, tmp_path, name):
    circuit = CIRCUITS[name]
    want = sr.zkey(circuit, sr.TRAPDOOR, None)                    # all-zero points: what the host writes on its own
    secs = sr.sections(want)
    path = tmp_path / "c.r1cs"
    path.write_bytes(write(circuit))
    n_wires, rowsA, rowsB, _, n_pub_out, n_pub_in = circuit
    n_public, M = n_pub_out + n_pub_in, len(rowsA)
    records = sum(len(r) for r in rowsA) + sum(len(r) for r in rowsB) + n_public + 1
    assert run(exe, "shape", path) == [
        "rc=0",
        "wires=%d public=%d M=%d N=%d records=%d total=%d" % (n_wires, n_public, M, sr.domain(M, n_public), records, len(want)),
        " ".join(str(len(secs[k])) for k in range(1, 11))]
    out = tmp_path / "frame.zkey"
    assert run(exe, "frame", path, out) == ["ok"]
    got = out.read_bytes()
    assert got == want
    assert list(sr.sections(got)) == list(range(1, 11))           # sections 1 .. 10, in order


def test_toy_section_4_is_the_reference_made_keys(exe, tmp_path, toy_paths):
    path = tmp_path / "toy.r1cs"
    path.write_bytes(write(sr.TOY))
    out = tmp_path / "toy.zkey"
    assert run(exe, "frame", path, out) == ["ok"]
    golden = sr.sections(open(toy_paths[0], "rb").read())
    got = sr.sections(out.read_bytes())
    assert got[4] == golden[4]
    assert got[1] == golden[1] and got[2][:84] == golden[2][:84]  # protocol, and the header's integers: n8q q n8r r nVars nPublic N
    assert [len(got[k]) for k in range(1, 10)] == [len(golden[k]) for k in range(1, 10)]
    # the toy's layout (64-byte circuit hash, u32 number of contributions, the contributions) with none
    assert struct.unpack_from("<I", golden[10], 64)[0] == 1 and got[10] == bytes(64) + struct.pack("<I", 0)


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_every_term_lands_once_in_its_wire_row(exe, tmp_path, name):
    circuit = CIRCUITS[name]
    path = tmp_path / "c.r1cs"
    path.write_bytes(write(circuit))
    want = ["plan=0"]
    for r, row in enumerate(sr.columns(circuit)):
        while row and row[-1] == (0, 0):                          # indistinguishable from a slice's padding, and as harmless
            row = row[:-1]
        want.append(("%d :" % r) + "".join(" %d:%064x" % (c, k) for c, k in row))
    assert run(exe, "columns", path) == want


def test_long_rows_at_the_boundary_take_their_paths():
    """The model's own view of the shapes: the largest circuit has A-columns of exactly 64 and 65 terms and wire 0's column of
    B with one term per constraint."""
    circuit, _ = sr.mixed(*sr.MIXED_SHAPES[-1])
    n_wires = circuit[0]
    lens = sorted(len(r) for r in sr.columns(circuit))
    assert sr.SPMV_LONG in lens and sr.SPMV_LONG + 1 in lens and lens[-1] == 130
    assert len(sr.columns(circuit)[n_wires]) == 130               # wire 0 in every row of B
    assert not any(sr.columns(circuit)[m * n_wires + n_wires - 1] for m in range(3))   # a wire in no constraint


def test_refusals(exe, tmp_path):
    path = tmp_path / "empty.r1cs"
    path.write_bytes(rb.write(3, [], [], []))
    assert run(exe, "shape", path)[0] == "rc=%d" % ERR_ARG            # no constraint
    one = ([[(1, 1)]], [[(2, 1)]], [[(3, 1)]])
    limit = (1 << 32) // 3 + 1                                        # the first nWires with 3 * nWires >= 2^32
    path.write_bytes(rb.write(limit, *one, with_labels=False))
    assert run(exe, "shape", path)[0] == "rc=%d" % ERR_ARG
    path.write_bytes(rb.write(limit - 1, *one, with_labels=False))
    assert run(exe, "shape", path)[0] == "rc=0"
