"""CPU tests of the host side the three R1CS diagnostics share: keyless-zk-proofs_amd/csrc/r1cs_masks.h, from the bit masks a scan
leaves to counts, the ascending list cut at cap and the per-wire status bytes, and the closure's seed mask -- through
tests/cpp/r1cs_masks_check.cpp, a stand-alone program built with -fsanitize=address,undefined and run as a plain subprocess,
against a few lines of big-integer Python over the same masks.  Shapes: the 64-wire word edges, caps around the count, each output
pointer null in turn, bit 0 (ignored by the two scans, honoured as seed by the closure), stray bits at or above n_wires in the
last word, all-zero and all-one masks."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WIRES = (1, 2, 63, 64, 65, 127, 128, 129)
BOUND, ABSENT, UNBOUND, TWO_VALUED = 0, 1, 2, 3                       # include/k16.h K16_WIRE_*
SEED, DERIVED, DET_ABSENT, OPEN = 0, 1, 2, 3                          # include/k16.h K16_DET_*
PATTERN = 0xA5A5A5A5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("masks_host") / "r1cs_masks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_masks_check.cpp"), "-o", out], timeout=600)
    return out


def run(exe, tmp_path, cases):
    """cases: [(input line, expected output line)], all in one run of the program"""
    path = tmp_path / "cases.txt"
    path.write_text("".join(c + "\n" for c, _ in cases))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]     # the sanitizers stay silent
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (case, want), got in zip(cases, lines):
        assert got == want, case


def n_words(n):
    return (n + 63) // 64


def hexwords(mask, n):
    return " ".join("%x" % ((mask >> (64 * w)) & (2 ** 64 - 1)) for w in range(n_words(n)))


def shown(name, values):
    return " %s=%s" % (name, "-" if values is None else ",".join("%x" % v for v in values))


def listed(wires, cap, there, pattern=PATTERN):
    """a list output of `cap` places: the lowest wires, the pattern behind them; None for a null pointer"""
    return (wires[:cap] + [pattern] * (cap - min(cap, len(wires)))) if there else None


def masks_for(n, rng):
    """(present, mask) pairs as whole words -- stray bits above n_wires included: all zero, all one, and random ones with bit 0
    of the mask set and clear"""
    full = 2 ** (64 * n_words(n)) - 1
    rnd = lambda: rng.getrandbits(64 * n_words(n))
    return [(0, 0), (full, full), (full, 0), (0, full), (rnd(), rnd() | 1), (rnd() | 1, rnd() & ~1)]


def caps(count):
    return sorted({c for c in (0, 1, count - 1, count, count + 1) if c >= 0})


def unbound_case(n, present, bound, cap, outs):
    free = [i for i in range(1, n) if not (bound >> i) & 1]
    cls = lambda i: UNBOUND if (present >> i) & 1 else ABSENT
    want = "absent=%d unbound=%d" % (sum(cls(i) == ABSENT for i in free), sum(cls(i) == UNBOUND for i in free))
    lists = bool(outs & 3)                                            # with both list outputs null nothing is listed
    want += shown("wires", listed(free if lists else [], cap, outs & 1))
    want += shown("class", listed([cls(i) for i in free] if lists else [], cap, outs & 2, 0xA5))
    want += shown("status", [cls(i) if i in set(free) else BOUND for i in range(n)] if outs & 4 else None)
    return "unbound %d %d %d %s %s" % (n, cap, outs, hexwords(present, n), hexwords(bound, n)), want


def second_case(n, present, pinned, rooted, cap, outs):
    two = [i for i in range(1, n) if (rooted >> i) & 1 and not (pinned >> i) & 1]
    free = [i for i in range(1, n) if not ((rooted | pinned) >> i) & 1]
    want = "two=%d listed=%d" % (len(two), min(cap, len(two)) if outs & 1 else 0)
    want += shown("wires", listed(two, cap, outs & 1))
    status = [TWO_VALUED if i in set(two) else (UNBOUND if (present >> i) & 1 else ABSENT) if i in set(free) else BOUND for i in range(n)]
    want += shown("status", status if outs & 4 else None)
    return "second %d %d %d %s %s %s" % (n, cap, outs, hexwords(present, n), hexwords(pinned, n), hexwords(rooted, n)), want


def closure_case(n, present, seed, known, cap, outs):
    got = [i for i in range(n) if (known >> i) & 1 and not (seed >> i) & 1]
    out = [i for i in range(n) if not (known >> i) & 1]
    opened = [i for i in out if (present >> i) & 1]
    want = "derived=%d absent=%d open=%d" % (len(got), len(out) - len(opened), len(opened))
    want += shown("wires", listed(opened, cap, outs & 1))
    want += shown("round", [0 if (seed >> i) & 1 else 7 for i in range(n)] if outs & 8 else None)   # round 0 for the seed, the rest stays
    status = [SEED if (seed >> i) & 1 else DERIVED if (known >> i) & 1 else OPEN if (present >> i) & 1 else DET_ABSENT for i in range(n)]
    want += shown("status", status if outs & 4 else None)
    return "closure %d %d %d %s %s %s" % (n, cap, outs, hexwords(present, n), hexwords(seed, n), hexwords(known, n)), want


def test_unbound_masks(exe, tmp_path):
    rng, cases = random.Random(1), []
    for n in N_WIRES:
        for present, bound in masks_for(n, rng):
            count = len([i for i in range(1, n) if not (bound >> i) & 1])
            for cap in caps(count):
                for outs in (7, 6, 5, 3, 4, 0):                       # each pointer null in turn; both lists; all
                    cases.append(unbound_case(n, present, bound, cap, outs))
    run(exe, tmp_path, cases)


def test_second_value_masks(exe, tmp_path):
    rng, cases = random.Random(2), []
    for n in N_WIRES:
        for present, pinned in masks_for(n, rng):
            for rooted in (0, 2 ** (64 * n_words(n)) - 1, rng.getrandbits(64 * n_words(n)) | 1):
                count = len([i for i in range(1, n) if (rooted >> i) & 1 and not (pinned >> i) & 1])
                for cap in caps(count):
                    for outs in (5, 4, 1, 0):
                        cases.append(second_case(n, present, pinned, rooted, cap, outs))
    run(exe, tmp_path, cases)


def test_closure_masks(exe, tmp_path):
    rng, cases = random.Random(3), []
    for n in N_WIRES:
        for present, known in masks_for(n, rng):
            for seed in (1, known | 1, known & rng.getrandbits(64 * n_words(n)) | 1, rng.getrandbits(64 * n_words(n))):
                count = len([i for i in range(n) if not (known >> i) & 1 and (present >> i) & 1])
                for cap in caps(count):
                    for outs in (13, 12, 9, 5, 0):
                        cases.append(closure_case(n, present, seed, known, cap, outs))
    run(exe, tmp_path, cases)


def test_seed_masks(exe, tmp_path):
    cases = []
    untouched = lambda n: shown("seed", [0x5A5A5A5A5A5A5A5A] * n_words(n))

    def seeded(n, wires):
        mask = 1                                                       # wire 0, always
        for i in wires:
            mask |= 1 << i
        return "refused=-" + shown("seed", [(mask >> (64 * w)) & (2 ** 64 - 1) for w in range(n_words(n))])

    for n in N_WIRES:
        # the header's inputs, 1 | outputs | public inputs | private inputs: up to exactly n_wires, and one beyond it
        for po, pi, pr in ((0, 0, 0), (0, 0, n - 1), (n - 1, 0, 0), ((n - 1) // 3, (n - 1) // 3, n - 1 - 2 * ((n - 1) // 3))):
            cases.append(("seed %d %d %d %d default" % (n, po, pi, pr), seeded(n, range(po + 1, po + 1 + pi + pr))))
            if po + 1 + pi + pr < n:
                continue
            cases.append(("seed %d %d %d %d default" % (n, po, pi, pr + 1),
                          "refused=the header's input wires reach beyond nWires" + untouched(n)))
            cases.append(("seed %d %d %d %d default" % (n, po + 1, pi, pr),
                          "refused=the header's input wires reach beyond nWires" + untouched(n)))
        # a list of the caller's: empty, wire 0 in it or not, a duplicate, the highest wire, any order; the header is not looked at
        for wires in ([], [0], [n - 1], [n - 1, 0, n - 1], [n // 2, n - 1, n // 2, 0, n // 2], list(range(n))[::-1]):
            cases.append(("seed %d %d %d %d list %d %s" % (n, n, n, n, len(wires), " ".join(map(str, wires))), seeded(n, wires)))
        for wires in ([n], [0, n - 1, n], [0xFFFFFFFF], [n + 63, 0]):
            cases.append(("seed %d 0 0 0 list %d %s" % (n, len(wires), " ".join(map(str, wires))),
                          "refused=seed wire number out of range" + untouched(n)))
    run(exe, tmp_path, cases)
