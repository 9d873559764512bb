"""CPU tests of keyless-zk-proofs_amd/csrc/r1cs_file.h -- the .r1cs reader, the layout plan of its 3 M rows and
r1cs_match_zkey -- through tests/cpp/r1cs_file_check.cpp, a stand-alone program built with -fsanitize=address,undefined and run
as a plain subprocess.  Files come from tests/r1cs_builder.py; the one pin that is not written by our own writer is the
reference-made tests/golden/toy/toy_1.zkey, whose section 4 must be the one-constraint circuit -w1 * w2 = -6."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pymodel as pm
import r1cs_builder as rb
import valid_key_builder as vkb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pm.R
OK, ERR_ARG, ERR_FORMAT, ERR_CURVE = 0, -3, -5, -6
DIFF_HEADER, DIFF_A, DIFF_B, DIFF_PUBLIC = 1, 2, 3, 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("r1cs_host") / "r1cs_file_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_file_check.cpp"), "-o", out], timeout=600)
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]     # the sanitizers stay silent
    return out.stdout.splitlines()


def put(tmp_path, name, raw):
    p = tmp_path / name
    p.write_bytes(raw)
    return p


def rc_of(exe, tmp_path, raw):
    return int(run(exe, "dump", put(tmp_path, "case.r1cs", raw))[0].split("=")[1])


def rand_row(rng, n_wires, n):
    return [(rng.next() % n_wires, rng.below(R)) for _ in range(n)]


def circuit(lengths, n_wires, seed):
    """Rows whose lengths walk through `lengths`, differently in each matrix."""
    rng = pm.SplitMix64(seed)
    m = len(lengths)
    return [[rand_row(rng, n_wires, lengths[(c + k) % m]) for c in range(m)] for k in range(3)]


def expected_dump(n_wires, rows, n_pub_in=0):
    rowsA = rows[0]
    terms = sum(len(r) for mat in rows for r in mat)
    lines = ["rc=0", "wires=%d pub_out=0 pub_in=%d prv_in=%d labels=%d constraints=%d public=%d terms=%d"
             % (n_wires, n_pub_in, max(0, n_wires - 1 - n_pub_in), n_wires, len(rowsA), n_pub_in, terms)]
    for name, mat in zip("ABC", rows):
        for c, row in enumerate(mat):
            lines.append(("%s %d :" % (name, c)) + "".join(" %d:%064x" % (w, k) for w, k in row))
    return lines + ["plan=0"]


CIRCUITS = {
    "empty": (3, [[], [], []]),
    "one": (3, [[[(1, R - 1)]], [[(2, 1)]], [[(0, R - 6)]]]),
    "edges": (300, circuit([0, 1, 63, 64, 65, 200], 300, seed=5)),
    "duplicate_wire": (4, [[[(1, 5), (2, 7), (1, R - 5), (1, 9)]], [[(3, 1), (3, 1)]], [[]]]),
    "many_slices": (50, circuit([2, 0, 3, 1, 64, 65] * 40, 50, seed=6)),
}


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_files_parse_to_the_rows_written_and_every_term_is_placed_once(exe, tmp_path, name):
    n_wires, rows = CIRCUITS[name]
    raw = rb.write(n_wires, *rows)
    assert run(exe, "dump", put(tmp_path, "c.r1cs", raw)) == expected_dump(n_wires, rows)
    raw = rb.write(n_wires, *rows, n_pub_in=1, with_labels=False)              # no section 3: it is ignored anyway
    assert run(exe, "dump", put(tmp_path, "c.r1cs", raw)) == expected_dump(n_wires, rows, n_pub_in=1)


def test_plan_limits_and_field_helpers(exe):
    assert run(exe, "selftest") == ["ok"]


def test_every_documented_error(exe, tmp_path):
    n_wires, rows = 4, [[[(1, 2), (3, 4)], [(2, 1)]], [[(2, 3)], []], [[(0, 5)], [(1, 1)]]]
    hdr = rb.header(n_wires, 0, 1, 2, n_wires, 2)
    body = rb.constraints(*rows)
    good = rb.container([(1, hdr), (2, body)])
    assert rc_of(exe, tmp_path, good) == OK
    first_count = good.index(body)                                               # constraint 0, A: u32 n = 2

    def with_body(b, h=hdr):
        return rb.container([(1, h), (2, b)])

    fmt = {
        "truncated file": good[:-1],
        "truncated inside a coefficient": good[:first_count + 20],
        "section shorter than its counts imply": with_body(body[:-36]),
        "count past the section": with_body(struct.pack("<I", 7) + body[4:]),         # 7 x 36 > the 236 bytes behind it
        "huge count": with_body(struct.pack("<I", 0xFFFFFFFF) + body[4:]),
        "wire = nWires": with_body(rb.constraints([[(4, 2)], []], [[], []], [[], []])),
        "coefficient = r": with_body(rb.constraints([[(1, R)], []], [[], []], [[], []])),
        "coefficient = 2^256 - 1": with_body(rb.constraints([[(1, 2 ** 256 - 1)], []], [[], []], [[], []])),
        "trailing bytes in section 2": with_body(body + b"\0"),
        "a whole extra constraint": with_body(body + rb.constraints([[]], [[]], [[]])),
        "M larger than the section": with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, 3)),
        "short header": rb.container([(1, hdr[:-1]), (2, body)]),
        "no header": rb.container([(2, body)]),
        "no constraints": rb.container([(1, hdr)]),
        "bad magic": b"r1cx" + good[4:],
        "version 2": rb.container([(1, hdr), (2, body)], version=2),
        "section runs past the file": good[:12] + struct.pack("<IQ", 1, 1 << 40) + good[24:],
        "more public wires than wires": with_body(body, rb.header(n_wires, 2, 2, 0, n_wires, 2)),
    }
    for what, raw in fmt.items():
        assert rc_of(exe, tmp_path, raw) == ERR_FORMAT, what
    curve = {
        "fieldSize 31": with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, 2, field_size=31, prime=R >> 8)),
        "fieldSize 64": with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, 2, field_size=64)),
        "prime = BN254 q": with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, 2, prime=pm.Q)),
        "prime = r + 2": with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, 2, prime=R + 2)),
    }
    for what, raw in curve.items():
        assert rc_of(exe, tmp_path, raw) == ERR_CURVE, what
    m_limit = (2 ** 32 + 2) // 3                                                 # the smallest M with 3 M >= 2^32
    assert rc_of(exe, tmp_path, with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, m_limit))) == ERR_ARG
    assert rc_of(exe, tmp_path, with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, 0xFFFFFFFF))) == ERR_ARG
    assert rc_of(exe, tmp_path, with_body(body, rb.header(n_wires, 0, 1, 2, n_wires, m_limit - 1))) == ERR_FORMAT
    # the first occurrence of a section type wins; unknown sections are skipped
    twice = rb.container([(7, b"junk"), (1, hdr), (2, body), (2, body + b"\0"), (1, hdr[:-1])])
    assert run(exe, "dump", put(tmp_path, "t.r1cs", twice)) == expected_dump(n_wires, rows, n_pub_in=1)


def test_truncations_and_byte_corruptions_parse_or_are_refused(exe, tmp_path):
    rows = circuit([0, 1, 2, 3, 1], 9, seed=8)
    raw = rb.write(9, *rows, n_pub_in=2)
    assert 900 <= len(raw) <= 1500
    out = run(exe, "mutate", put(tmp_path, "m.r1cs", raw))
    assert out[-1].startswith("ok parsed="), out
    parsed, refused = (int(x.split("=")[1]) for x in out[-1].split()[1:])
    assert parsed > 100 and refused > len(raw)                                   # both outcomes occur, every truncation is refused


def match(exe, tmp_path, r1cs, zkey):
    line = run(exe, "match", put(tmp_path, "m.r1cs", r1cs), put(tmp_path, "m.zkey", zkey))[0]
    return tuple(int(x.split("=")[1]) for x in line.split())


def test_match_zkey_toy_pair_made_by_the_reference(exe, tmp_path, toy_paths):
    zkey = open(toy_paths[0], "rb").read()
    toy = rb.write(3, [[(1, R - 1)]], [[(2, 1)]], [[(0, R - 6)]], n_pub_out=1)
    assert match(exe, tmp_path, toy, zkey) == (OK, 0, 0, 0)
    assert rb.check([[(1, R - 1)]], [[(2, 1)]], [[(0, R - 6)]], [1, 2, 3]) == []  # and toy.wtns = (1, 2, 3) satisfies it
    assert match(exe, tmp_path, rb.write(3, [[(1, 1)]], [[(2, 1)]], [[(0, 6)]], n_pub_out=1), zkey) == (OK, DIFF_A, 0, 1)
    assert match(exe, tmp_path, rb.write(3, [[(1, R - 1)]], [[(1, 1)]], [[(0, R - 6)]], n_pub_out=1), zkey) == (OK, DIFF_B, 0, 1)
    assert match(exe, tmp_path, rb.write(3, [[(1, R - 1)]], [[(2, 1)]], [[(0, R - 6)]]), zkey)[:2] == (OK, DIFF_HEADER)
    assert match(exe, tmp_path, toy, zkey[:len(zkey) // 2])[0] == ERR_FORMAT
    assert match(exe, tmp_path, toy, toy)[0] == ERR_FORMAT


def no_points(group, scalars):
    """r1cs_match_zkey reads the header and section 4 only: the point sections of this key are blank."""
    return np.zeros((len(scalars), 64 if group == 0 else 128), dtype=np.uint8)


def edit_section4(zkey, fn):
    """The zkey with its coefficient records (list of [m, c, s, value bytes]) passed through fn."""
    nsec = struct.unpack_from("<I", zkey, 8)[0]
    pos, out = 12, []
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", zkey, pos)
        payload = zkey[pos + 12:pos + 12 + size]
        if typ == 4:
            n = struct.unpack_from("<I", payload, 0)[0]
            recs = [list(struct.unpack_from("<III", payload, 4 + 44 * i)) + [payload[16 + 44 * i:48 + 44 * i]] for i in range(n)]
            recs = fn(recs)
            payload = struct.pack("<I", len(recs)) + b"".join(struct.pack("<III", *r[:3]) + r[3] for r in recs)
        out.append(struct.pack("<IQ", typ, len(payload)) + payload)
        pos += 12 + size
    return zkey[:12] + b"".join(out)


def test_match_zkey_builder_pair_and_every_kind_of_difference(exe, tmp_path):
    key = vkb.build(no_points, n_bits=20, n_bytes=4, n_prod=30, seed=4)
    n_wires, rowsA, rowsB, rowsC, n_pub = rb.from_shape(key["shape"])
    M = len(rowsA)
    good = rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_in=n_pub)
    assert match(exe, tmp_path, good, key["zkey"]) == (OK, 0, 0, 0)
    assert rb.check(rowsA, rowsB, rowsC, rb.witness_ints(key["witness"])) == []
    c = M - 3                                                                    # a product row: A = k1 w_a + k2 w_b
    (wa, ka), rest = rowsA[c][0], rowsA[c][1:]

    def variant(A=rowsA, B=rowsB, nw=n_wires):
        return rb.write(nw, A, B, rowsC, n_pub_in=n_pub)

    coef = [r if i != c else [(wa, ka + 1)] + rest for i, r in enumerate(rowsA)]
    assert match(exe, tmp_path, variant(A=coef), key["zkey"]) == (OK, DIFF_A, c, wa)
    other = next(w for w in range(n_wires) if w not in [t[0] for t in rowsA[c]])
    moved = [r if i != c else [(other, ka)] + rest for i, r in enumerate(rowsA)]
    assert match(exe, tmp_path, variant(A=moved), key["zkey"]) == (OK, DIFF_A, c, min(other, wa))
    wb = rowsB[5][0][0]                                                          # a bit row: B = w_i - w_0
    movedB = [r if i != 5 else [(wb + 1, 1), (0, R - 1)] for i, r in enumerate(rowsB)]
    assert match(exe, tmp_path, variant(B=movedB), key["zkey"]) == (OK, DIFF_B, 5, wb)
    assert match(exe, tmp_path, variant(A=rowsB, B=rowsA), key["zkey"]) == (OK, DIFF_A, 0, 0)   # bit row 0: B has wire 0, A has not
    assert match(exe, tmp_path, variant(nw=n_wires + 1), key["zkey"])[:2] == (OK, DIFF_HEADER)
    # a wire listed twice adds up: 3 w + (k - 3) w is the same row
    split = [r if i != c else [(wa, 3), (wa, (ka - 3) % R)] + rest for i, r in enumerate(rowsA)]
    assert match(exe, tmp_path, variant(A=split), key["zkey"]) == (OK, 0, 0, 0)
    # differences on the key's side: the row of public wire 1 missing; a coefficient of B changed; a stray record
    no_pub = edit_section4(key["zkey"], lambda recs: [r for r in recs if not (r[0] == 0 and r[1] == M + 1)])
    assert match(exe, tmp_path, good, no_pub) == (OK, DIFF_PUBLIC, M + 1, 1)
    wrong_pub = edit_section4(key["zkey"], lambda recs: [r if r[1] != M else [0, M, 1, r[3]] for r in recs])
    assert match(exe, tmp_path, good, wrong_pub) == (OK, DIFF_PUBLIC, M, 0)

    def bump_b(recs):
        i = next(i for i, r in enumerate(recs) if r[0] == 1 and r[1] == 7)
        recs[i][3] = ((int.from_bytes(recs[i][3], "little") + 1) % R).to_bytes(32, "little")
        return recs
    assert match(exe, tmp_path, good, edit_section4(key["zkey"], bump_b))[:3] == (OK, DIFF_B, 7)

    def not_canonical(recs):                                                     # the same value as r + itself: equals nothing
        i = next(i for i, r in enumerate(recs) if r[0] == 1 and r[1] == 7)
        recs[i][3] = (int.from_bytes(recs[i][3], "little") + R).to_bytes(32, "little")
        return recs
    assert match(exe, tmp_path, good, edit_section4(key["zkey"], not_canonical))[:3] == (OK, DIFF_B, 7)
    zero_as_r = edit_section4(key["zkey"], lambda recs: recs + [[0, 3, 0, R.to_bytes(32, "little")]])
    assert match(exe, tmp_path, good, zero_as_r) == (OK, DIFF_A, 3, 0)
    stray = edit_section4(key["zkey"], lambda recs: recs + [[1, M, 0, recs[0][3]]])
    assert match(exe, tmp_path, good, stray)[:3] == (OK, DIFF_B, M)
