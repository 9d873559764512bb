"""Checked proving (include/k16.h: k16_prover_set_r1cs, k16_prover_last_check, k16_fullprover_set_r1cs,
k16_fullprover_last_rejection) where no GPU is needed: null objects and a FullProver that is not ready get status codes,
never a crash; a thread that never proved has no rejection."""
import ctypes
import threading

from test_boundary import LIB

ERR_NO_DEVICE, ERR_ARG = -1, -3
CHECK_NONE = 0


def lib():
    L = ctypes.CDLL(LIB)
    L.k16_prover_set_r1cs.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.k16_prover_last_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    L.k16_fullprover_set_r1cs.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.k16_fullprover_last_rejection.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    return L


def test_null_prover_is_refused():
    L = lib()
    status, n = ctypes.c_int(7), ctypes.c_uint64(7)
    out = (ctypes.c_uint32 * 4)()
    assert L.k16_prover_set_r1cs(None, None) == ERR_ARG
    assert L.k16_prover_set_r1cs(None, ctypes.c_void_p(0x1234)) == ERR_ARG     # (the object is never looked at)
    assert L.k16_prover_last_check(None, ctypes.byref(status), ctypes.byref(n), out, 4) == ERR_ARG
    assert (status.value, n.value) == (7, 7)


def test_fullprover_that_is_not_ready():
    L = lib()

    class Fields(ctypes.Structure):                      # include/k16_fullprover.hpp: { FullProverImpl* impl; FullProverState state; }
        _fields_ = [("impl", ctypes.c_void_p), ("state", ctypes.c_int)]

    fp = Fields(None, 1)
    assert L.k16_fullprover_set_r1cs(ctypes.byref(fp), b"/nonexistent/circuit.r1cs") == ERR_NO_DEVICE
    assert L.k16_fullprover_set_r1cs(ctypes.byref(fp), None) == ERR_NO_DEVICE
    assert L.k16_fullprover_set_r1cs(None, None) == ERR_NO_DEVICE


def test_a_thread_that_never_proved_has_no_rejection():
    L = lib()
    got = []

    def ask():
        status, n = ctypes.c_int(7), ctypes.c_uint64(7)
        out = (ctypes.c_uint32 * 64)(*([9] * 64))
        rc = L.k16_fullprover_last_rejection(ctypes.byref(n), out, 64, ctypes.byref(status))
        got.append((rc, status.value, n.value, list(out)))
        assert L.k16_fullprover_last_rejection(None, out, 64, ctypes.byref(status)) == ERR_ARG
        assert L.k16_fullprover_last_rejection(ctypes.byref(n), None, 0, None) == ERR_ARG

    ask()
    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert got == [(0, CHECK_NONE, 0, [9] * 64)] * 2
