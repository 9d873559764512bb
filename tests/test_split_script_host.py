"""CPU: the split check's two programs (csrc/verify_script.h, coop_build_early_program / coop_build_late_program) executed
on the host with the concrete field for random points: late(early(A, B, vk_x), C) is the GT value of the straight-line
code and of the single per-proof program, final_exponentiation(early) is that of the two-pair product, and the step
counts say how much of the check moves under the prover's H MSM (tests/cpp/split_script_check.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_programs_on_host_equal_single_program_and_straight_line_code(tmp_path):
    exe = str(tmp_path / "ssc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "split_script_check.cpp"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("split GT value identical") == 3 and "MISMATCH" not in out.stdout
    m = re.search(r"steps: single (\d+) early (\d+) late (\d+)", out.stdout)
    single, early, late = (int(x) for x in m.groups())
    # what has to wait for C is less than the whole check; what runs under the H MSM is no more than the Miller part
    assert 0 < late < single and 0 < early < single and early + late < 2 * single
