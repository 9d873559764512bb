"""The point checks of keyless-zk-proofs_amd/csrc/bn254_points.h are __host__ __device__ templates on the field type: this
compiles the same sequence the kernels of points_check.hip run (host code only, no GPU) on the canonical field (Fq2) and on
the radix-2^29 field (Fq2n), and compares every status with the definitional class of tests/subgroup_fixtures.py
([r] Q = O over pymodel's affine arithmetic)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import subgroup_fixtures as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("subgroup") / "subgroup_check")
    # -O0: the host build of these inlined templates takes minutes at -O2 and the run is a fraction of a second either way
    subprocess.check_call([HIPCC, "-O0", "-std=c++17", "-x", "hip", "--offload-host-only",
                           "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "subgroup_check.cpp"), "-o", exe], timeout=600)
    return exe


def _run(exe, tmp_path, mode, pts):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(pts).tofile(fin)
    out = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK %d" % len(pts)), out.stdout + out.stderr
    return np.fromfile(fout, dtype=np.uint8)


def test_fixture_classes_are_definitional():
    """The fixture set holds what the checks must tell apart, each class asserted by [r] Q = O."""
    pts, want, small = sf.g2_fixtures()
    assert len(pts) >= 200 and small.sum() >= 20
    assert (want[small] == sf.NOT_IN_SUBGROUP).all()
    for c in (sf.OK, sf.NONCANONICAL, sf.OFF_CURVE, sf.NOT_IN_SUBGROUP):
        assert (want == c).sum() >= 10, c


def test_g2_subgroup_sequence_on_the_host(check_exe, tmp_path):
    pts, want, small = sf.g2_fixtures()
    got = _run(check_exe, tmp_path, "g2", pts).reshape(-1, 2)
    for col, field in enumerate(("Fq2", "Fq2n")):
        bad = np.nonzero(got[:, col] != want)[0]
        assert bad.size == 0, "%s: points %s got %s want %s" % (field, bad[:10], got[bad[:10], col], want[bad[:10]])
    assert (got[small, 1] == sf.NOT_IN_SUBGROUP).all()


def test_g1_point_status_on_the_host(check_exe, tmp_path):
    pts, want = sf.g1_fixtures()
    got = _run(check_exe, tmp_path, "g1", pts)
    assert (got == want).all(), (got, want)
