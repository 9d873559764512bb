"""The reference of the determinism closure and its certificate replayer (tests/determined_reference.py) on circuits worked by
hand, and the argument checks of the binding that need no device.  No GPU.  The host-only code of k16_r1cs_determined_wires
(the seed mask and the walk over the closure's masks, csrc/r1cs_masks.h) has its stand-alone C++ program in
tests/test_r1cs_masks_host.py."""
import pytest

import determined_reference as dr
import second_value_reference as sv
from determined_reference import ABSENT, DERIVED, NONE, OPEN, SEED


def solved(name):
    circuit, w, header, seed = dr.resolved(dr.DIRECTED[name])
    return (circuit, w, seed) + dr.closure(circuit, w, seed)


@pytest.mark.parametrize("name", sorted(dr.EXPECTED))
def test_reference_on_hand_worked_circuits(name):
    circuit, w, seed, status, rounds, by = solved(name)
    for wire, want in dr.EXPECTED[name].items():
        assert (status[wire], rounds[wire], by[wire]) == want, wire
    assert (status[0], rounds[0], by[0]) == (SEED, 0, NONE)
    assert dr.replay(circuit, w, seed, status, rounds, by) is None


def test_chain_rounds():
    circuit, w, seed, status, rounds, by = solved("chain_300")
    assert rounds == [0, 0] + list(range(1, 301)) and by == [NONE, NONE] + list(range(300))
    assert dr.summary(status, rounds) == (300, 0, 0, 300, [])


@pytest.mark.parametrize("name", sorted(dr.DIRECTED))
def test_every_directed_certificate_replays(name):
    circuit, w, seed, status, rounds, by = solved(name)
    assert dr.replay(circuit, w, seed, status, rounds, by) is None
    n_derived, n_absent, n_open, n_rounds, opened = dr.summary(status, rounds)
    assert n_derived + n_absent + n_open + len(set(seed) | {0}) == circuit[0]
    assert sorted(set(rounds) - {NONE}) == list(range(n_rounds + 1))    # no level is empty


def test_default_seed_is_the_headers_inputs():
    assert dr.default_seed((2, 3, 4)) == [0, 3, 4, 5, 6, 7, 8, 9]
    assert dr.default_seed((0, 0, 0)) == [0]


def test_the_moving_pair_is_what_the_single_wire_scans_miss():
    """both wires are single-valued for the second-value scan, yet open here: the pair moves together"""
    circuit, w, seed, status, rounds, by = solved("moving_pair")
    classes, shifts = sv.classify(*circuit, w)
    assert classes[1] == sv.BOUND and classes[3] == sv.TWO_VALUED       # tmp alone has its other root; out alone is pinned
    assert status[1] == status[3] == OPEN
    w2 = list(w)
    w2[3], w2[1] = 9, 81                                                # another witness under the same input
    assert sv.residuals(*circuit[1:], w2) == [0] and w2[2] == w[2]


def test_replayer_rejects_a_round_too_low():
    circuit, w, seed, status, rounds, by = solved("chain_3")
    rounds = list(rounds)
    rounds[4] = 2                                                       # as low as the wire it is derived from
    assert "not known before" in dr.replay(circuit, w, seed, status, rounds, by)


def test_replayer_rejects_a_wrong_constraint():
    circuit, w, seed, status, rounds, by = solved("delayed")
    by = list(by)
    by[5] = 1                                                           # holds only one round later: wire 3 is round 2 too
    assert "not known before" in dr.replay(circuit, w, seed, status, rounds, by)
    by[5] = 3                                                           # a constraint the wire is not in
    assert "is not in constraint" in dr.replay(circuit, w, seed, status, rounds, by)


def test_replayer_rejects_a_root_passed_as_a_pin():
    circuit, w, seed, status, rounds, by = solved("square_root_at_3")
    assert status[2] == OPEN
    status, rounds, by = list(status), list(rounds), list(by)
    status[2], rounds[2], by[2] = DERIVED, 1, 0
    assert "is no PIN" in dr.replay(circuit, w, seed, status, rounds, by)


def test_replayer_rejects_a_broken_constraint_and_loose_ends():
    circuit, w, seed, status, rounds, by = solved("broken_link")
    status, rounds, by = list(status), list(rounds), list(by)
    status[3], rounds[3], by[3] = DERIVED, 2, 1
    assert "is broken" in dr.replay(circuit, w, seed, status, rounds, by)
    circuit, w, seed, status, rounds, by = solved("moving_pair")
    rounds = list(rounds)
    rounds[1] = 1                                                       # an open wire with a round
    assert "neither seed nor derived" in dr.replay(circuit, w, seed, status, rounds, by)


def test_random_cases_are_not_degenerate():
    """what the GPU test asserts of the same cases, so that a change of the generator shows here first"""
    good = 0
    for i in range(dr.N_RANDOM):
        circuit, w, header, seed = dr.resolved(dr.random_case(i))
        status, rounds, by = dr.closure(circuit, w, seed)
        assert dr.replay(circuit, w, seed, status, rounds, by) is None, i
        good += status.count(DERIVED) > 0 and status.count(OPEN) > 0
    assert good >= 30


class _NoDevice:
    """stands where an R1cs object's context would: any call into the library is a failure of the test"""
    class L:
        @staticmethod
        def k16_r1cs_determined_wires(*a):
            raise AssertionError("reached the library")

        @staticmethod
        def k16_r1cs_info(h, nw, npub, m, nt):
            nw._obj.value = 5
            return 0

    @staticmethod
    def _chk(rc):
        assert rc == 0


def test_binding_refuses_bad_arguments_before_the_library():
    import k16
    assert (k16.DET_SEED, k16.DET_DERIVED, k16.DET_ABSENT, k16.DET_OPEN, k16.DET_NONE) == (SEED, DERIVED, ABSENT, OPEN, NONE)
    assert "k16_r1cs_determined_wires" in k16.SYMBOLS
    circ = k16.R1cs.__new__(k16.R1cs)
    circ.ctx, circ.h = _NoDevice, None
    for seed in ([-1], [1 << 32], [1, 2, -3]):
        with pytest.raises(ValueError):
            circ.determined_wires(seed=seed)
    with pytest.raises(ValueError):
        circ.determined_wires(cap=-1)
    with pytest.raises((TypeError, ValueError)):
        circ.determined_wires(seed=["x"])
