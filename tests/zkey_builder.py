"""Builds synthetic Groth16 .zkey / .wtns files in the iden3 binary container format the prover parses
(rust-rapidsnark/rapidsnark/src/binfile_utils.cpp:13-58, zkey_utils.hpp:49-87,
wtns_utils.hpp:29-44).  The "circuit" is random: the proof will not verify, but prove() is a deterministic
function of (zkey, witness, r, s), which is what the parity tests compare between the HIP path and the oracle.
"""
import struct

import numpy as np

import oracle_lib as ol
import pymodel as pm


def _section(t, payload):
    return struct.pack("<IQ", t, len(payload)) + payload


def _write_zkey(path, n_vars, n_public, domain_size, coef_section, rs, zero_frac):
    """Header, point sections and container around a finished coefficient section (section 4).  rs: the RandomState that
    zeroes B1 / B2 columns; build_zkey hands over the one its coefficients came from."""
    g1 = ol.gen_points(ol.G1, 100, 6)          # alpha1, beta1, delta1 + spare
    g2 = ol.gen_points(ol.G2, 50, 3)           # beta2, gamma2, delta2
    hdr = struct.pack("<I", 32) + pm.limbs(pm.Q) + struct.pack("<I", 32) + pm.limbs(pm.R)
    hdr += struct.pack("<III", n_vars, n_public, domain_size)
    hdr += bytes(g1[0]) + bytes(g1[1]) + bytes(g2[0]) + bytes(g2[1]) + bytes(g1[2]) + bytes(g2[2])

    def pts(group, start, n, zf):
        p = ol.gen_points(group, start, n)
        if n and zf > 0:
            p[rs.rand(n) < zf] = 0              # sparse B1/B2 columns are (0,0) in real keys
        return p.tobytes()

    secs = [
        _section(1, struct.pack("<I", 1)),
        _section(2, hdr),
        _section(3, bytes(ol.gen_points(ol.G1, 7, n_public + 1).tobytes())),
        _section(4, bytes(coef_section)),
        _section(5, pts(ol.G1, 1000, n_vars, 0.0)),
        _section(6, pts(ol.G1, 200000, n_vars, zero_frac)),
        _section(7, pts(ol.G2, 3000, n_vars, zero_frac)),
        _section(8, pts(ol.G1, 400000, n_vars - n_public - 1, 0.0)),
        _section(9, pts(ol.G1, 600000, domain_size, 0.0)),
    ]
    with open(path, "wb") as f:
        f.write(b"zkey" + struct.pack("<II", 1, len(secs)) + b"".join(secs))


def build_zkey(path, n_vars, n_public, domain_size, n_coefs, seed=1, zero_frac=0.3, long_rows=()):
    """long_rows: lengths of extra constraint rows of one matrix each (65 ... thousands of entries, as circom's Num2Bits or
    a wide linear combination produce); their coefficients are part of n_coefs and keep the file sorted by constraint."""
    rs = np.random.RandomState(seed)
    # coefficients: (m, c, s, value * R^2 mod r), grouped by c then m as snarkjs writes them
    m = rs.randint(0, 2, size=n_coefs).astype(np.uint32)
    c = rs.randint(0, domain_size, size=n_coefs).astype(np.uint32)
    at = 0
    for k, ln in enumerate(long_rows):          # one (m, c) row gets ln entries
        assert at + ln <= n_coefs
        c[at:at + ln] = (k * 7919 + 5) % domain_size
        m[at:at + ln] = k & 1
        at += ln
    order = np.argsort(c, kind="stable")
    c, m = c[order], m[order]
    s = rs.randint(0, n_vars, size=n_coefs).astype(np.uint32)
    r2 = pow(pm.MONT, 2, pm.R)
    coefs = bytearray(struct.pack("<I", n_coefs))
    for i in range(n_coefs):
        v = int(rs.randint(1, 1 << 30)) if rs.rand() < 0.7 else pm.SplitMix64(seed * 7919 + i).below(pm.R)
        coefs += struct.pack("<III", int(m[i]), int(c[i]), int(s[i])) + pm.limbs(v * r2 % pm.R)
    _write_zkey(path, n_vars, n_public, domain_size, coefs, rs, zero_frac)


COEF_DTYPE = np.dtype([("m", "<u4"), ("c", "<u4"), ("s", "<u4"), ("v", "u1", (32,))])   # 44 bytes, packed


def coef_section(matrix, constraint, wire, value, sort_by=("c", "m")):
    """Section 4 of a .zkey from explicit rows.  matrix / constraint / wire: integer sequences of one length; value: the
    coefficients as Python integers in [0, r) (standard form; the file holds value * R^2 mod r as snarkjs writes it).
    sort_by: ("c", "m") orders the list by constraint, then matrix, entries of one row in the order given (stable);
    ("c",) by constraint alone; () keeps the order given.  Only the distinct values go through big-integer arithmetic, the
    records are assembled with numpy."""
    m = np.asarray(matrix, dtype=np.uint32)
    c = np.asarray(constraint, dtype=np.uint32)
    s = np.asarray(wire, dtype=np.uint32)
    n = len(m)
    assert len(c) == n and len(s) == n and len(value) == n
    r2 = pow(pm.MONT, 2, pm.R)
    lut = {}
    idx = np.fromiter((lut.setdefault(int(v), len(lut)) for v in value), dtype=np.int64, count=n)
    assert all(0 <= v < pm.R for v in lut), "coefficients are field elements in standard form"
    table = np.frombuffer(b"".join(pm.limbs(v * r2 % pm.R) for v in lut), dtype=np.uint8).reshape(-1, 32) if lut else \
        np.zeros((0, 32), dtype=np.uint8)
    rec = np.zeros(n, dtype=COEF_DTYPE)
    rec["m"], rec["c"], rec["s"] = m, c, s
    rec["v"] = table[idx]
    if sort_by:
        keys = {"c": c, "m": m}
        rec = rec[np.lexsort(tuple(keys[k] for k in reversed(sort_by)))]     # lexsort: last key is the primary one
    return struct.pack("<I", n) + rec.tobytes()


def build_zkey_rows(path, n_vars, n_public, domain_size, matrix, constraint, wire, value, seed=1, zero_frac=0.3, rs=None,
                    sort_by=("c", "m")):
    """build_zkey with the coefficient list given explicitly instead of drawn (see coef_section): the same iden3 container,
    the same point sections.  rs: RandomState for the zeroed B1 / B2 columns (default: RandomState(seed))."""
    c = np.asarray(constraint, dtype=np.int64)
    s = np.asarray(wire, dtype=np.int64)
    m = np.asarray(matrix, dtype=np.int64)
    assert len(c) == 0 or (0 <= c.min() and c.max() < domain_size and 0 <= s.min() and s.max() < n_vars and 0 <= m.min())
    _write_zkey(path, n_vars, n_public, domain_size, coef_section(matrix, constraint, wire, value, sort_by),
                rs if rs is not None else np.random.RandomState(seed), zero_frac)


def build_wtns(path, n_vars, seed=2):
    """90 % bits, 8 % bytes, 2 % full-width field elements; w[0] = 1."""
    rs = np.random.RandomState(seed)
    w = np.zeros((n_vars, 32), dtype=np.uint8)
    u = rs.rand(n_vars)
    w[u < 0.90, 0] = rs.randint(0, 2, size=int((u < 0.90).sum()))
    byts = (u >= 0.90) & (u < 0.98)
    w[byts, 0] = rs.randint(0, 256, size=int(byts.sum()))
    full = np.nonzero(u >= 0.98)[0]
    for k, i in enumerate(full):
        w[i] = np.frombuffer(pm.limbs(pm.SplitMix64(seed * 104729 + k).below(pm.R)), dtype=np.uint8)
    w[0] = 0
    w[0, 0] = 1
    write_wtns(path, w)
    return w


def write_wtns(path, w):
    """An explicit witness as a .wtns file.  w: uint8 array (n_vars, 32), little-endian values in standard form, or a
    sequence of Python integers in [0, r).  Returns the uint8 array."""
    if not (isinstance(w, np.ndarray) and w.dtype == np.uint8):
        assert all(0 <= int(v) < pm.R for v in w), "witness values are field elements in standard form"
        w = np.frombuffer(b"".join(pm.limbs(int(v)) for v in w), dtype=np.uint8).reshape(-1, 32)
    assert w.ndim == 2 and w.shape[1] == 32
    sec1 = struct.pack("<I", 32) + pm.limbs(pm.R) + struct.pack("<I", w.shape[0])
    with open(path, "wb") as f:
        f.write(b"wtns" + struct.pack("<II", 2, 2) + _section(1, sec1) + _section(2, np.ascontiguousarray(w).tobytes()))
    return w
