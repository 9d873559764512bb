"""Writes iden3 .r1cs files from per-row term lists, rebuilds the circuit of valid_key_builder.build(...)['shape'] as such
rows, and holds the reference checker of the R1CS witness check (Python big integers, row by row).

A circuit here is (n_wires, rowsA, rowsB, rowsC): three lists of M rows, each row a list of (wire, coefficient) with the
coefficient an int in [0, r).  Constraint c holds for w when <A_c, w> * <B_c, w> = <C_c, w> mod r.

Container (csrc/r1cs_file.h): magic "r1cs", u32 version 1, u32 nSections, then { u32 type, u64 size, payload } per section;
section 1 = header, 2 = constraints, 3 = wire -> label map (written as the identity, ignored by the reader)."""
import struct

import numpy as np

import pymodel as pm

R = pm.R


def _section(t, payload):
    return struct.pack("<IQ", t, len(payload)) + payload


def _lc(row):
    return struct.pack("<I", len(row)) + b"".join(struct.pack("<I", w) + int(k).to_bytes(32, "little") for w, k in row)


def header(n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, m, field_size=32, prime=R):
    return (struct.pack("<I", field_size) + int(prime).to_bytes(field_size, "little") +
            struct.pack("<IIIIQI", n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, m))


def constraints(rowsA, rowsB, rowsC):
    return b"".join(_lc(a) + _lc(b) + _lc(c) for a, b, c in zip(rowsA, rowsB, rowsC))


def container(sections, version=1):
    return b"r1cs" + struct.pack("<II", version, len(sections)) + b"".join(_section(t, p) for t, p in sections)


def write(n_wires, rowsA, rowsB, rowsC, n_pub_out=0, n_pub_in=0, n_prv_in=None, with_labels=True):
    """The .r1cs file of a circuit as bytes."""
    assert len(rowsA) == len(rowsB) == len(rowsC)
    if n_prv_in is None:
        n_prv_in = max(0, n_wires - 1 - n_pub_out - n_pub_in)
    secs = [(2, constraints(rowsA, rowsB, rowsC)),            # "in any order": the header is not first
            (1, header(n_wires, n_pub_out, n_pub_in, n_prv_in, n_wires, len(rowsA)))]
    if with_labels:
        secs.append((3, np.arange(n_wires, dtype="<u8").tobytes()))
    return container(secs)


def from_shape(shape):
    """(n_wires, rowsA, rowsB, rowsC, n_pub_in) of valid_key_builder's circuit: the bit rows, then the product rows; the
    rows snarkjs appends for the public wires exist in the zkey only."""
    rowsA, rowsB, rowsC = [], [], []
    for i in range(shape["bit0"], shape["byte0"]):
        rowsA.append([(i, 1)])
        rowsB.append([(i, 1), (0, R - 1)])
        rowsC.append([])
    for c, a, b, d, k1, k2, k3 in shape["prods"]:
        rowsA.append([(a, k1), (b, k2)] if a != b else [(a, (k1 + k2) % R)])
        rowsB.append([(d, k3)])
        rowsC.append([(c, 1)])
    return shape["n_vars"], rowsA, rowsB, rowsC, 1


def write_from_shape(shape):
    n_wires, rowsA, rowsB, rowsC, n_pub_in = from_shape(shape)
    return write(n_wires, rowsA, rowsB, rowsC, n_pub_in=n_pub_in)


def dot(row, w):
    return sum(k * w[s] for s, k in row) % R


def values(rowsA, rowsB, rowsC, w, c):
    """(A.w, B.w, C.w) of constraint c, canonical."""
    return dot(rowsA[c], w), dot(rowsB[c], w), dot(rowsC[c], w)


def check(rowsA, rowsB, rowsC, w):
    """The reference checker: the broken constraints of the assignment w (ints), ascending."""
    return [c for c in range(len(rowsA)) if dot(rowsA[c], w) * dot(rowsB[c], w) % R != dot(rowsC[c], w)]


def witness_bytes(w):
    """n x 32 uint8, standard form little-endian (any 256-bit ints: refusals are tested with values >= r)."""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in w), dtype=np.uint8).reshape(len(w), 32).copy()


def witness_ints(wb):
    return [int.from_bytes(wb[i].tobytes(), "little") for i in range(wb.shape[0])]
