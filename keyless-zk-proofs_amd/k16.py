"""ctypes binding of libk16.so (include/k16.h) -- used by tests/, bench.py and __graft_entry__.py.

There is deliberately no fallback: if the HIP library is missing or no GPU is present,
loading / context creation raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("K16_LIB_PATH") or os.path.join(HERE, "libk16.so")  # override: A/B-testing builds

G1, G2 = 0, 1
OPT_PIPELINED_MSM = 1
OPT_GRAPHS = 2
OPT_SHARED_GPU = 3
OPT_YIELDING_WAITS = 4
FQ, FR = 0, 1
FQ9, FR9, FQ2N, FQ2H = 2, 3, 4, 5          # the same ops on the hot kernels' radix-2^29 representations (include/k16.h)
G1_ENG9, G2_ENG2N, G2_PAIR = 2, 3, 4
OP_ADD, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_TOMONT, OP_FROMMONT, OP_LAZY_ADDMUL, OP_LAZY_SUBMUL = range(9)
PT_ADD, PT_MADD, PT_DBL, PT_MADD_ACC = range(4)
AFF_BYTES = {G1: 64, G2: 128, G1_ENG9: 64, G2_ENG2N: 128, G2_PAIR: 128}
XYZZ_BYTES = {G1: 128, G2: 256, G1_ENG9: 128, G2_ENG2N: 256, G2_PAIR: 256}


def op_bound(op, ka=0, kb=0):
    """K16_OP_BOUND_A / _B: operands moved up by ka / kb multiples of the modulus (radix-2^29 selectors only)."""
    return op | (ka << 8) | (kb << 12)

ERR = {0: "OK", -1: "NO_DEVICE", -2: "HIP", -3: "ARG", -4: "IO", -5: "FORMAT", -6: "CURVE", -7: "BUFFER", -8: "NOMEM"}

# every symbol include/k16.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "k16_runtime_hw_queues", "k16_device_count", "k16_host_threads", "k16_ctx_create", "k16_ctx_create_ex", "k16_ctx_destroy", "k16_last_error", "k16_sync", "k16_stream",
    "k16_dev_alloc", "k16_dev_free", "k16_h2d", "k16_d2h", "k16_host_register", "k16_host_unregister",
    "k16_timer_start", "k16_timer_stop", "k16_kernel_stats_enable", "k16_kernel_stats_reset", "k16_kernel_stats_get",
    "k16_ctx_set_option", "k16_msm", "k16_msm_host", "k16_msm_enqueue", "k16_msm_finish", "k16_msm_finish_group", "k16_msm_pending", "k16_msm_abort_all", "k16_msm_bases_prepare", "k16_msm_enqueue_prepared", "k16_msm_fixed_base_info", "k16_msm_fixed_base_prepare", "k16_msm_enqueue_fixed_base", "k16_msm_set_window_bits", "k16_msm_set_lane", "k16_points_sum",
    "k16_msm_zero_row_mask", "k16_msm_set_zero_row_mask", "k16_msm_sort_from_lane", "k16_scalar_classes_create", "k16_scalar_classes_destroy", "k16_scalar_classes_build", "k16_scalar_classes_counts", "k16_msm_enqueue_classified",
    "k16_ntt", "k16_ntt_host", "k16_synth_points", "k16_synth_points_scalars", "k16_field_op_vec", "k16_point_op_vec", "k16_coop_exec",
    "k16_prover_create", "k16_prover_create_mem", "k16_prover_create_shared", "k16_prover_destroy", "k16_prover_info",
    "k16_prover_prove_file", "k16_prover_prove_file_timed", "k16_prover_prove_mem", "k16_prover_compact_buffers", "k16_prover_prove_compact", "k16_fullprover_prove_mem", "k16_fullprover_compact_lease", "k16_fullprover_prove_compact", "k16_fullprover_compact_cancel", "k16_prover_last_h", "k16_prover_warmup_status",
    "k16_vk_create", "k16_vk_destroy", "k16_verify_batch", "k16_verify_coop_gt", "k16_pairing_vec",
    "k16_points_check", "k16_verify_batch_checked", "k16_zkey_check", "k16_zkey_check_file",
    "k16_verify_batch_folded", "k16_verify_fold_gt",
    "k16_vk_create_from_zkey", "k16_vk_create_from_zkey_file", "k16_prover_set_vk", "k16_prover_prove_mem_verified",
    "k16_prover_prove_compact_verified", "k16_prover_prove_file_verified", "k16_verify_split_gt", "k16_fullprover_set_verify",
    "k16_r1cs_create", "k16_r1cs_create_mem", "k16_r1cs_destroy", "k16_r1cs_info", "k16_r1cs_check_mem", "k16_r1cs_check_file",
    "k16_r1cs_check_prover_witness", "k16_r1cs_last_values", "k16_r1cs_match_zkey",
    "k16_r1cs_unbound_wires", "k16_r1cs_wire_constraints", "k16_r1cs_incidences", "k16_r1cs_second_values",
    "k16_r1cs_determined_wires", "k16_r1cs_complete_witness", "k16_r1cs_complete_witness_ex", "k16_r1cs_boolean_wires",
    "k16_r1cs_determined_wires_ex", "k16_r1cs_held_wires", "k16_r1cs_open_system", "k16_r1cs_open_direction",
    "k16_r1cs_open_system_ex", "k16_r1cs_open_direction_ex",
    "k16_prover_set_r1cs", "k16_prover_last_check", "k16_fullprover_set_r1cs", "k16_fullprover_last_rejection",
    "k16_r1cs_setup_size", "k16_r1cs_setup", "k16_r1cs_setup_file", "k16_generator_mul", "k16_generator_mul_info",
    "k16_msm_sharded_create", "k16_msm_sharded_destroy", "k16_msm_sharded_count", "k16_msm_sharded_range", "k16_msm_sharded_ctx",
    "k16_msm_sharded_last_error", "k16_msm_sharded_set_bases", "k16_msm_sharded_set_bases_device", "k16_msm_sharded_run",
    "k16_msm_sharded_run_device", "k16_msm_sharded_set_piece_rows", "k16_msm_sharded_last_ms",
    "k16_rank_comm_unique_id", "k16_rank_comm_load_error", "k16_rank_comm_create", "k16_rank_comm_destroy", "k16_rank_comm_allgather_fold", "k16_rank_comm_allgather_start", "k16_rank_comm_allgather_finish",
]

_lib = None


class K16Error(RuntimeError):
    def __init__(self, rc, msg=""):
        super().__init__("k16 error %s (%d) %s" % (ERR.get(rc, "?"), rc, msg))
        self.rc = rc


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise K16Error(-1, "libk16.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, u64, i32, u32, sz = C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_size_t
    L.k16_runtime_hw_queues.argtypes = [i32]
    L.k16_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.k16_ctx_create_ex.argtypes = [i32, i32, C.POINTER(vp)]
    L.k16_ctx_destroy.argtypes = [vp]
    L.k16_ctx_destroy.restype = None
    L.k16_last_error.argtypes = [vp]
    L.k16_last_error.restype = C.c_char_p
    L.k16_sync.argtypes = [vp]
    L.k16_stream.argtypes = [vp]
    L.k16_stream.restype = vp
    L.k16_dev_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.k16_dev_free.argtypes = [vp, vp]
    L.k16_h2d.argtypes = [vp, vp, vp, sz]
    L.k16_d2h.argtypes = [vp, vp, vp, sz]
    L.k16_host_register.argtypes = [vp, vp, sz]
    L.k16_host_unregister.argtypes = [vp, vp]
    L.k16_timer_start.argtypes = [vp]
    L.k16_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    L.k16_kernel_stats_enable.argtypes = [vp, i32]
    L.k16_kernel_stats_reset.argtypes = [vp]
    L.k16_kernel_stats_get.argtypes = [vp, C.c_char_p, C.POINTER(u64), C.POINTER(C.c_double)]
    L.k16_ctx_set_option.argtypes = [vp, i32, i32]
    L.k16_msm.argtypes = [vp, i32, vp, vp, u64, vp, vp]
    L.k16_msm_host.argtypes = [vp, i32, vp, vp, u64, vp, vp]
    L.k16_msm_enqueue.argtypes = [vp, i32, vp, vp, u64]
    L.k16_msm_finish.argtypes = [vp, vp, vp]
    L.k16_msm_finish_group.argtypes = [vp, i32, vp, vp]
    L.k16_msm_pending.argtypes = [vp]
    L.k16_msm_abort_all.argtypes = [vp]
    L.k16_msm_bases_prepare.argtypes = [vp, i32, vp, u64, vp]
    L.k16_msm_enqueue_prepared.argtypes = [vp, i32, vp, vp, u64]
    L.k16_msm_fixed_base_info.argtypes = [u64, C.POINTER(u32), C.POINTER(u64)]
    L.k16_msm_fixed_base_prepare.argtypes = [vp, i32, vp, u64, vp]
    L.k16_msm_enqueue_fixed_base.argtypes = [vp, i32, vp, vp, u64]
    L.k16_msm_set_window_bits.argtypes = [vp, u32]
    L.k16_msm_set_lane.argtypes = [vp, i32]
    L.k16_points_sum.argtypes = [i32, vp, u64, vp, vp]
    L.k16_msm_zero_row_mask.argtypes = [vp, i32, vp, u64, vp]
    L.k16_msm_set_zero_row_mask.argtypes = [vp, vp]
    L.k16_msm_sort_from_lane.argtypes = [vp, i32, i32]
    L.k16_scalar_classes_create.argtypes = [vp, u64, i32, C.POINTER(vp)]
    L.k16_scalar_classes_destroy.argtypes = [vp]
    L.k16_scalar_classes_destroy.restype = None
    L.k16_scalar_classes_build.argtypes = [vp, vp, vp, u64, C.POINTER(vp), i32, C.c_int64]
    L.k16_scalar_classes_counts.argtypes = [vp, vp, vp]
    L.k16_msm_enqueue_classified.argtypes = [vp, i32, vp, vp, i32]
    L.k16_ntt.argtypes = [vp, vp, u64, u64, i32]
    L.k16_ntt_host.argtypes = [vp, vp, u64, u64, i32]
    L.k16_synth_points.argtypes = [vp, i32, u64, u64, vp]
    L.k16_synth_points_scalars.argtypes = [vp, i32, vp, u64, vp]
    L.k16_field_op_vec.argtypes = [vp, i32, i32, vp, vp, vp, u64]
    L.k16_point_op_vec.argtypes = [vp, i32, i32, vp, vp, vp, u64]
    L.k16_coop_exec.argtypes = [vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp, u64, vp]
    L.k16_prover_create.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.k16_prover_create_mem.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.k16_prover_create_shared.argtypes = [vp, vp, C.POINTER(vp)]
    L.k16_prover_destroy.argtypes = [vp]
    L.k16_prover_destroy.restype = None
    L.k16_prover_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
    L.k16_prover_prove_file.argtypes = [vp, C.c_char_p, vp, vp, C.c_char_p, sz, C.POINTER(C.c_float)]
    L.k16_prover_prove_file_timed.argtypes = [vp, C.c_char_p, vp, vp, C.c_char_p, sz, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.k16_prover_prove_mem.argtypes = [vp, vp, u64, vp, vp, C.c_char_p, sz, C.POINTER(C.c_float)]
    L.k16_prover_compact_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.k16_prover_prove_compact.argtypes = [vp, u64, vp, vp, C.c_char_p, sz, C.POINTER(C.c_float)]
    L.k16_prover_last_h.argtypes = [vp, vp]
    L.k16_fullprover_prove_mem.argtypes = [vp, vp, u64, C.c_char_p, sz, C.POINTER(i32)]
    L.k16_fullprover_compact_lease.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u32)]
    L.k16_fullprover_prove_compact.argtypes = [vp, vp, u64, C.c_char_p, sz, C.POINTER(i32)]
    L.k16_fullprover_compact_cancel.argtypes = [vp, vp]
    L.k16_prover_warmup_status.argtypes = [vp]
    L.k16_vk_create.argtypes = [vp, vp, vp, vp, vp, vp, u32, C.POINTER(vp)]
    L.k16_vk_destroy.argtypes = [vp]
    L.k16_vk_destroy.restype = None
    L.k16_verify_batch.argtypes = [vp, vp, vp, vp, u64, vp]
    L.k16_verify_coop_gt.argtypes = [vp, vp, vp, vp, u64, vp]
    L.k16_pairing_vec.argtypes = [vp, vp, vp, u64, vp]
    L.k16_points_check.argtypes = [vp, i32, vp, u64, vp]
    L.k16_verify_batch_checked.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.k16_verify_batch_folded.argtypes = [vp, vp, vp, vp, u64, vp, vp, C.POINTER(C.c_uint8)]
    L.k16_verify_fold_gt.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.k16_vk_create_from_zkey.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.k16_vk_create_from_zkey_file.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.k16_prover_set_vk.argtypes = [vp, vp]
    L.k16_prover_prove_mem_verified.argtypes = [vp, vp, u64, vp, vp, C.c_char_p, sz, C.POINTER(C.c_float), vp, C.POINTER(C.c_uint8)]
    L.k16_prover_prove_compact_verified.argtypes = [vp, u64, vp, vp, C.c_char_p, sz, C.POINTER(C.c_float), vp, C.POINTER(C.c_uint8)]
    L.k16_prover_prove_file_verified.argtypes = [vp, C.c_char_p, vp, vp, C.c_char_p, sz, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, C.POINTER(C.c_uint8)]
    L.k16_fullprover_set_verify.argtypes = [vp, i32]
    L.k16_verify_split_gt.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.k16_zkey_check.argtypes = [vp, vp, sz, C.POINTER(u32), C.POINTER(u64), C.POINTER(C.c_uint8), C.POINTER(u64)]
    L.k16_zkey_check_file.argtypes = [vp, C.c_char_p, C.POINTER(u32), C.POINTER(u64), C.POINTER(C.c_uint8), C.POINTER(u64)]
    L.k16_r1cs_create.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.k16_r1cs_create_mem.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.k16_r1cs_destroy.argtypes = [vp]
    L.k16_r1cs_destroy.restype = None
    L.k16_r1cs_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
    L.k16_r1cs_check_mem.argtypes = [vp, vp, vp, u64, C.POINTER(u64), vp, u32]
    L.k16_r1cs_check_file.argtypes = [vp, vp, C.c_char_p, C.POINTER(u64), vp, u32]
    L.k16_r1cs_check_prover_witness.argtypes = [vp, vp, C.POINTER(u64), vp, u32]
    L.k16_r1cs_last_values.argtypes = [vp, u32, vp]
    L.k16_r1cs_match_zkey.argtypes = [vp, vp, vp, sz, C.POINTER(u32)]
    L.k16_r1cs_unbound_wires.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), vp, vp, u32, vp]
    L.k16_r1cs_wire_constraints.argtypes = [vp, u32, C.POINTER(u64), vp, u32]
    L.k16_r1cs_incidences.argtypes = [vp, C.POINTER(u64)]
    L.k16_r1cs_second_values.argtypes = [vp, C.POINTER(u64), vp, vp, u32, vp]
    L.k16_r1cs_determined_wires.argtypes = [vp, vp, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), vp, u32,
                                            vp, vp, vp]
    L.k16_r1cs_complete_witness.argtypes = [vp, vp, vp, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32),
                                            C.POINTER(u64), vp, u32, C.POINTER(u64), vp, u32, vp, vp, vp]
    L.k16_r1cs_complete_witness_ex.argtypes = [vp, vp, vp, u32, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32),
                                               C.POINTER(u64), vp, u32, C.POINTER(u64), vp, u32, vp, vp, vp, C.POINTER(u64),
                                               C.POINTER(u64), vp, u32, vp]
    L.k16_r1cs_boolean_wires.argtypes = [vp, C.POINTER(u64), vp]
    L.k16_r1cs_determined_wires_ex.argtypes = [vp, vp, u32, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), vp, u32,
                                               vp, vp, vp, C.POINTER(u64), vp]
    L.k16_r1cs_held_wires.argtypes = [vp, C.POINTER(u64), vp]
    L.k16_r1cs_open_system.argtypes = [vp, vp] + [C.POINTER(u64)] * 7 + [vp, vp, u32, vp, vp]
    L.k16_r1cs_open_direction.argtypes = [vp, vp, u32, C.POINTER(C.c_uint8)] + [C.POINTER(u32)] * 4 + [C.POINTER(u64), vp, vp, u32]
    L.k16_r1cs_open_system_ex.argtypes = [vp, vp, u32] + [C.POINTER(u64)] * 7 + [vp, vp, u32, vp, vp]
    L.k16_r1cs_open_direction_ex.argtypes = [vp, vp, u32, u32, C.POINTER(C.c_uint8)] + [C.POINTER(u32)] * 4 + [C.POINTER(u64), vp, vp, u32]
    L.k16_prover_set_r1cs.argtypes = [vp, vp]
    L.k16_prover_last_check.argtypes = [vp, C.POINTER(i32), C.POINTER(u64), vp, u32]
    L.k16_fullprover_set_r1cs.argtypes = [vp, C.c_char_p]
    L.k16_fullprover_last_rejection.argtypes = [C.POINTER(u64), vp, u32, C.POINTER(i32)]
    L.k16_r1cs_setup_size.argtypes = [vp, C.POINTER(u64)]
    L.k16_r1cs_setup.argtypes = [vp, vp, vp, vp, sz, C.POINTER(sz)]
    L.k16_r1cs_setup_file.argtypes = [vp, vp, vp, C.c_char_p]
    L.k16_generator_mul.argtypes = [vp, i32, vp, u64, vp]
    L.k16_generator_mul_info.argtypes = [i32, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.k16_msm_sharded_create.argtypes = [C.POINTER(i32), i32, i32, u64, C.POINTER(vp)]
    L.k16_msm_sharded_destroy.argtypes = [vp]
    L.k16_msm_sharded_destroy.restype = None
    L.k16_msm_sharded_count.argtypes = [vp]
    L.k16_msm_sharded_range.argtypes = [vp, i32, C.POINTER(u64), C.POINTER(u64)]
    L.k16_msm_sharded_ctx.argtypes = [vp, i32]
    L.k16_msm_sharded_ctx.restype = vp
    L.k16_msm_sharded_last_error.argtypes = [vp]
    L.k16_msm_sharded_last_error.restype = C.c_char_p
    L.k16_msm_sharded_set_bases.argtypes = [vp, vp]
    L.k16_msm_sharded_set_bases_device.argtypes = [vp, i32, vp]
    L.k16_msm_sharded_run.argtypes = [vp, vp, vp, vp]
    L.k16_msm_sharded_run_device.argtypes = [vp, C.POINTER(vp), vp, vp]
    L.k16_msm_sharded_last_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.k16_msm_sharded_set_piece_rows.argtypes = [vp, u64, u64]
    L.k16_rank_comm_unique_id.argtypes = [vp]
    L.k16_rank_comm_load_error.argtypes = []
    L.k16_rank_comm_load_error.restype = C.c_char_p
    L.k16_rank_comm_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.k16_rank_comm_destroy.argtypes = [vp]
    L.k16_rank_comm_destroy.restype = None
    L.k16_rank_comm_allgather_fold.argtypes = [vp, i32, vp, vp, vp]
    L.k16_rank_comm_allgather_start.argtypes = [vp, i32, vp]
    L.k16_rank_comm_allgather_finish.argtypes = [vp, vp, vp]
    _lib = L
    return L


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return a


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        ctx._chk(ctx.L.k16_dev_alloc(ctx.h, nbytes, C.byref(p)))
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.L.k16_h2d(self.ctx.h, self.ptr, _p(arr), arr.nbytes))
        return self

    def download(self, dtype=np.uint8, shape=None):
        out = np.empty(self.nbytes, dtype=np.uint8)
        self.ctx._chk(self.ctx.L.k16_d2h(self.ctx.h, _p(out), self.ptr, self.nbytes))
        out = out.view(dtype)
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if self.ptr:
            self.ctx.L.k16_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    def __init__(self, device=0, stream_offset=0):
        """stream_offset: k16_ctx_create_ex -- placeholder streams created before the context's own (include/k16.h)"""
        self.L = load()
        h = C.c_void_p()
        rc = self.L.k16_ctx_create_ex(device, stream_offset, C.byref(h)) if stream_offset else self.L.k16_ctx_create(device, C.byref(h))
        if rc:
            raise K16Error(rc, "k16_ctx_create(device=%d): no usable HIP device" % device)
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            if not getattr(self, "borrowed", False):   # a ShardedMsm's contexts belong to it
                self.L.k16_ctx_destroy(self.h)
            self.h = None

    def _chk(self, rc):
        if rc:
            raise K16Error(rc, (self.L.k16_last_error(self.h) or b"").decode())

    def sync(self):
        self._chk(self.L.k16_sync(self.h))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, max(arr.nbytes, 16)).upload(arr)

    def host_register(self, arr):
        """page-lock a numpy array the caller keeps alive (k16_host_register): uploads from it are DMA copies"""
        assert arr.flags["C_CONTIGUOUS"]
        self._chk(self.L.k16_host_register(self.h, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def host_unregister(self, arr):
        self._chk(self.L.k16_host_unregister(self.h, arr.ctypes.data_as(C.c_void_p)))

    def timer_start(self):
        self._chk(self.L.k16_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.L.k16_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def stats_enable(self, on=True):
        self._chk(self.L.k16_kernel_stats_enable(self.h, int(on)))

    def stats_reset(self):
        self._chk(self.L.k16_kernel_stats_reset(self.h))

    def stats_get(self, name):
        n, ms = C.c_uint64(), C.c_double()
        self._chk(self.L.k16_kernel_stats_get(self.h, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def set_option(self, option, value):
        self._chk(self.L.k16_ctx_set_option(self.h, option, value))

    def set_lane(self, lane):
        self._chk(self.L.k16_msm_set_lane(self.h, lane))

    def set_window_bits(self, c):
        self._chk(self.L.k16_msm_set_window_bits(self.h, c))

    # ---- MSM
    def msm_device(self, group, d_bases, d_scalars, n):
        x = np.zeros(XYZZ_BYTES[group], dtype=np.uint8)
        a = np.zeros(AFF_BYTES[group], dtype=np.uint8)
        self._chk(self.L.k16_msm(self.h, group, d_bases.ptr if d_bases else None,
                                 d_scalars.ptr if d_scalars else None, n, _p(x), _p(a)))
        return x.tobytes(), a.tobytes()

    def msm_enqueue(self, group, d_bases, d_scalars, n):
        self._chk(self.L.k16_msm_enqueue(self.h, group, d_bases.ptr, d_scalars.ptr, n))

    def bases_prepare(self, group, d_bases, n):
        out = self.alloc(max(n * AFF_BYTES[group], 16))
        self._chk(self.L.k16_msm_bases_prepare(self.h, group, d_bases.ptr, n, out.ptr))
        self.sync()
        return out

    def msm_enqueue_prepared(self, group, d_prepared, d_scalars, n):
        self._chk(self.L.k16_msm_enqueue_prepared(self.h, group, d_prepared.ptr, d_scalars.ptr, n))

    def fixed_base_prepare(self, group, d_bases, n):
        """Window tables for a static table (k16_msm_fixed_base_prepare). Returns (DeviceBuffer, c) or (None, 0) when
        this n has no fixed-base mode."""
        c, rows = C.c_uint32(0), C.c_uint64(0)
        self._chk(self.L.k16_msm_fixed_base_info(n, C.byref(c), C.byref(rows)))
        if c.value == 0:
            return None, 0
        out = self.alloc(rows.value * AFF_BYTES[group])
        self._chk(self.L.k16_msm_fixed_base_prepare(self.h, group, d_bases.ptr, n, out.ptr))
        self.sync()
        return out, c.value

    def msm_enqueue_fixed_base(self, group, d_table, d_scalars, n):
        self._chk(self.L.k16_msm_enqueue_fixed_base(self.h, group, d_table.ptr, d_scalars.ptr, n))

    # ---- scalar-class MSM (witness-like scalars)
    def zero_row_mask(self, group, d_rows, n):
        d = self.alloc(max((n + 63) // 64 * 8, 16))
        self._chk(self.L.k16_msm_zero_row_mask(self.h, group, d_rows.ptr, n, d.ptr))
        self.sync()
        return d

    def msm_set_zero_row_mask(self, d_mask):
        self._chk(self.L.k16_msm_set_zero_row_mask(self.h, d_mask.ptr if d_mask is not None else None))

    def msm_sort_from_lane(self, lane, derive=False):
        self._chk(self.L.k16_msm_sort_from_lane(self.h, lane, 1 if derive else 0))

    def classes_create(self, max_n, max_sets=1):
        h = C.c_void_p()
        self._chk(self.L.k16_scalar_classes_create(self.h, max_n, max_sets, C.byref(h)))
        return h

    def classes_destroy(self, cls):
        self.L.k16_scalar_classes_destroy(cls)

    def classes_build(self, cls, d_scalars, n, masks=None, n_wide_bound=-1):
        """masks: list of DeviceBuffer / None, one per set (None: one set, no zero rows)."""
        masks = masks if masks is not None else [None]
        arr = (C.c_void_p * len(masks))(*[(m.ptr if m is not None else None) for m in masks])
        self._chk(self.L.k16_scalar_classes_build(self.h, cls, d_scalars.ptr if d_scalars else None, n, arr, len(masks), n_wide_bound))

    def classes_counts(self, cls, n_sets):
        out = np.zeros(n_sets * 8 + 1, dtype=np.uint32)
        self._chk(self.L.k16_scalar_classes_counts(self.h, cls, _p(out)))
        return out

    def msm_enqueue_classified(self, group, d_prepared, cls, set_index=0):
        self._chk(self.L.k16_msm_enqueue_classified(self.h, group, d_prepared.ptr if d_prepared else None, cls, set_index))

    def msm_finish(self, group):
        x = np.zeros(XYZZ_BYTES[group], dtype=np.uint8)
        a = np.zeros(AFF_BYTES[group], dtype=np.uint8)
        self._chk(self.L.k16_msm_finish_group(self.h, group, _p(x), _p(a)))   # refuses a result of the other group
        return x.tobytes(), a.tobytes()

    def msm_pending(self):
        return self.L.k16_msm_pending(self.h)

    def msm_abort_all(self):
        self._chk(self.L.k16_msm_abort_all(self.h))

    def msm(self, group, bases, scalars):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8)
        n = scalars.shape[0] if scalars.ndim == 2 else 0
        x = np.zeros(XYZZ_BYTES[group], dtype=np.uint8)
        a = np.zeros(AFF_BYTES[group], dtype=np.uint8)
        self._chk(self.L.k16_msm_host(self.h, group, _p(bases), _p(scalars), n, _p(x), _p(a)))
        return x.tobytes(), a.tobytes()

    def points_check(self, group, pts):
        """Status of every encoded point (k16_points_check): pts (n, 64) for G1 / (n, 128) for G2 affine Montgomery, or
        raw bytes -> (n,) uint8 of PT_OK / PT_NONCANONICAL / PT_OFF_CURVE / PT_NOT_IN_SUBGROUP."""
        a = np.frombuffer(pts, dtype=np.uint8) if isinstance(pts, (bytes, bytearray)) else np.ascontiguousarray(pts, dtype=np.uint8)
        n = a.size // AFF_BYTES[group]
        assert a.size == n * AFF_BYTES[group]
        st = np.zeros(n, dtype=np.uint8)
        self._chk(self.L.k16_points_check(self.h, group, _p(a) if n else None, n, _p(st) if n else None))
        return st

    def synth_points(self, group, start, n):
        """Device buffer with (start+i+1)*G, i < n (affine Montgomery)."""
        d = self.alloc(max(n * AFF_BYTES[group], 16))
        self._chk(self.L.k16_synth_points(self.h, group, start, n, d.ptr))
        self.sync()
        return d

    def generator_mul(self, group, scalars):
        """k16_generator_mul: scalars = list of ints below 2^256 (NOT reduced: any 256-bit value is legal), or an (n, 32) uint8
        array of little-endian values -> uint8 array (n, AFF_BYTES) of scalar_i * G through the generator's window table."""
        return self._scalar_points(self.L.k16_generator_mul, group, scalars)

    def synth_points_scalars_raw(self, group, scalars):
        """k16_synth_points_scalars on the scalars as they are (generator_mul's argument forms)."""
        return self._scalar_points(self.L.k16_synth_points_scalars, group, scalars)

    def _scalar_points(self, call, group, scalars):
        if isinstance(scalars, np.ndarray):
            buf = np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1)
        else:
            buf = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in scalars), dtype=np.uint8)
        n = buf.size // 32
        if n == 0:
            return np.zeros((0, AFF_BYTES[group]), dtype=np.uint8)
        d_s = self.to_device(buf)
        d_o = self.alloc(n * AFF_BYTES[group])
        try:
            self._chk(call(self.h, group, d_s.ptr, n, d_o.ptr))
            self.sync()
            return d_o.download(np.uint8, (n, AFF_BYTES[group])).copy()
        finally:
            d_s.free()
            d_o.free()

    def synth_points_scalars(self, group, scalars):
        """scalars: list of ints (any size, reduced mod r here) -> uint8 array (n, AFF_BYTES) of scalar_i * G."""
        R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
        n = len(scalars)
        if n == 0:
            return np.zeros((0, AFF_BYTES[group]), dtype=np.uint8)
        buf = np.frombuffer(b"".join((int(k) % R_MOD).to_bytes(32, "little") for k in scalars), dtype=np.uint8)
        d_s = self.to_device(buf)
        d_o = self.alloc(n * AFF_BYTES[group])
        self._chk(self.L.k16_synth_points_scalars(self.h, group, d_s.ptr, n, d_o.ptr))
        self.sync()
        out = d_o.download(np.uint8, (n, AFF_BYTES[group])).copy()
        d_s.free()
        d_o.free()
        return out

    # ---- NTT
    def ntt(self, a, max_domain=None, inverse=False):
        a = np.ascontiguousarray(a, dtype=np.uint64).copy()
        n = a.shape[0]
        self._chk(self.L.k16_ntt_host(self.h, _p(a), n, max_domain or n, 1 if inverse else 0))
        return a

    def ntt_device(self, d_a, n, max_domain=None, inverse=False):
        self._chk(self.L.k16_ntt(self.h, d_a.ptr, n, max_domain or n, 1 if inverse else 0))

    # ---- batch primitives
    def field_op_vec(self, field, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        n = a.shape[0]
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.uint64)
        r = np.zeros_like(a)              # (n, 4) u64; (n, 8) for FQ2N elements
        self._chk(self.L.k16_field_op_vec(self.h, field, op, _p(a), _p(b), _p(r), n))
        return r

    def coop_exec(self, step_class, words, terms, n_const, n_slots, out_slot, const9, inputs):
        """k16_coop_exec (a test primitive): a caller's program through the wave-cooperative verifier's interpreter.
        step_class: uint8[n_steps]; words: uint64[n_steps * 64]; terms: uint32[]; const9: uint32[n_const, 9] raw limbs;
        inputs: uint8[n, 12, 32] canonical Montgomery Fq.  Returns uint8[n, 12, 32].  Raises K16Error(ARG) with the rule
        a malformed program breaks; nothing is launched then."""
        sc = np.ascontiguousarray(step_class, dtype=np.uint8)
        w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        t = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1)
        c9 = np.ascontiguousarray(const9, dtype=np.uint32).reshape(-1)
        os_ = np.ascontiguousarray(out_slot, dtype=np.uint32).reshape(-1)
        inp = np.ascontiguousarray(inputs, dtype=np.uint8).reshape(-1, 12, 32)
        if w.size != 64 * sc.size or os_.size != 12 or c9.size != 9 * int(n_const):
            raise K16Error(-3, "coop_exec: array sizes")
        out = np.zeros_like(inp)
        self._chk(self.L.k16_coop_exec(self.h, _p(sc), sc.size, _p(w), _p(t), t.size, int(n_const), int(n_slots), _p(os_), _p(c9),
                                       _p(inp), inp.shape[0], _p(out)))
        return out

    def point_op_vec(self, group, op, p1, p2=None):
        p1 = np.ascontiguousarray(p1, dtype=np.uint8)
        n = p1.shape[0]
        if p2 is not None:
            p2 = np.ascontiguousarray(p2, dtype=np.uint8)
        r = np.zeros((n, XYZZ_BYTES[group]), dtype=np.uint8)
        self._chk(self.L.k16_point_op_vec(self.h, group, op, _p(p1), _p(p2), _p(r), n))
        return r


def points_sum(group, parts):
    """parts: uint8 (k, XYZZ_BYTES). Host-side fold of per-shard partial MSM results."""
    L = load()
    parts = np.ascontiguousarray(parts, dtype=np.uint8)
    x = np.zeros(XYZZ_BYTES[group], dtype=np.uint8)
    a = np.zeros(AFF_BYTES[group], dtype=np.uint8)
    rc = L.k16_points_sum(group, _p(parts), parts.shape[0], _p(x), _p(a))
    if rc:
        raise K16Error(rc)
    return x.tobytes(), a.tobytes()


# k16_prover_last_check / k16_fullprover_last_rejection (include/k16.h)
R1CS_REPORT_MAX = 64
CHECK_NONE, CHECK_SATISFIED, CHECK_BROKEN, CHECK_WITNESS_REFUSED = 0, 1, 2, 3
WIRE_BOUND, WIRE_ABSENT, WIRE_UNBOUND, WIRE_TWO_VALUED = 0, 1, 2, 3
DET_SEED, DET_DERIVED, DET_ABSENT, DET_OPEN = 0, 1, 2, 3
DET_NONE = 0xFFFFFFFF
SOLVE_GIVEN, SOLVE_SOLVED, SOLVE_ABSENT, SOLVE_OPEN = 0, 1, 2, 3
SOLVE_RULE_LINEAR, SOLVE_RULE_BITS = 1, 2
DET_RULE_PIN, DET_RULE_BITS = 1, 2
OPEN_FIXED, OPEN_ABSENT, OPEN_FORCED, OPEN_FREE, OPEN_UNDECIDED, OPEN_SKIPPED = 0, 1, 2, 3, 4, 5
OPEN_MAX_WIRES = 64                                                         # include/k16.h K16_OPEN_MAX_WIRES
OPEN_MAX_WIRES_EX = 256                                                     # include/k16.h K16_OPEN_MAX_WIRES_EX
OPEN_NO_COMPONENT = 0xFFFFFFFF


def _max_wires(max_wires):
    """the cap of an _ex call as the uint32 the library judges: what does not fit one is passed as a value it refuses"""
    m = int(max_wires)
    return m if 0 <= m <= 0xFFFFFFFF else 0


def fullprover_set_r1cs(fullprover, r1cs_path):
    """k16_fullprover_set_r1cs on a FullProver object's address (int or c_void_p); r1cs_path None detaches.  Returns the status."""
    return int(load().k16_fullprover_set_r1cs(fullprover, str(r1cs_path).encode() if r1cs_path is not None else None))


def fullprover_last_rejection(cap=R1CS_REPORT_MAX):
    """k16_fullprover_last_rejection: (status, n_failed, lowest constraint numbers) of the calling thread's last prove through a
    FullProver; CHECK_NONE when the R1CS check did not reject it."""
    cap = int(cap)
    out = np.zeros(max(cap, 1), dtype=np.uint32)
    st, n = C.c_int32(), C.c_uint64()
    rc = load().k16_fullprover_last_rejection(C.byref(n), _p(out), cap, C.byref(st))
    if rc:
        raise K16Error(rc)
    return int(st.value), int(n.value), out[:min(int(n.value), cap, R1CS_REPORT_MAX)].tolist()


class Prover:
    """Mirror of the reference's FullProver(zkey).prove(wtns) (fullprover.hpp:52-64) over the C ABI."""

    def __init__(self, ctx, zkey_path, share_key_of=None):
        """share_key_of: another Prover of the same key on the same device -- k16_prover_create_shared (one resident key)"""
        self.ctx = ctx
        h = C.c_void_p()
        if share_key_of is not None:
            rc = ctx.L.k16_prover_create_shared(ctx.h, share_key_of.h, C.byref(h))
        else:
            rc = ctx.L.k16_prover_create(ctx.h, zkey_path.encode(), C.byref(h))
        if rc:
            raise K16Error(rc, (ctx.L.k16_last_error(ctx.h) or b"").decode())
        self.h = h

    def info(self):
        nv, npub, ds, nc = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_prover_info(self.h, C.byref(nv), C.byref(npub), C.byref(ds), C.byref(nc)))
        return dict(n_vars=nv.value, n_public=npub.value, domain_size=ds.value, n_coefs=nc.value)

    def prove_file(self, wtns_path, r=None, s=None):
        buf = C.create_string_buffer(4096)
        ms = C.c_float()
        R_ = np.frombuffer(bytes(r), dtype=np.uint8).copy() if r is not None else None
        S_ = np.frombuffer(bytes(s), dtype=np.uint8).copy() if s is not None else None
        rc = self.ctx.L.k16_prover_prove_file(self.h, wtns_path.encode(), _p(R_), _p(S_), buf, 4096, C.byref(ms))
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())
        self.last_device_ms = ms.value
        return buf.value.decode()

    def prove_mem(self, wtns, r=None, s=None):
        wtns = np.ascontiguousarray(wtns, dtype=np.uint8)
        n_vars = wtns.size // 32
        buf = C.create_string_buffer(4096)
        ms = C.c_float()
        R_ = np.frombuffer(bytes(r), dtype=np.uint8).copy() if r is not None else None
        S_ = np.frombuffer(bytes(s), dtype=np.uint8).copy() if s is not None else None
        rc = self.ctx.L.k16_prover_prove_mem(self.h, _p(wtns), n_vars, _p(R_), _p(S_), buf, 4096, C.byref(ms))
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())
        self.last_device_ms = ms.value
        return buf.value.decode()

    def compact_buffers(self):
        """The prover's pinned upload buffers as numpy views (k16_prover_compact_buffers): narrow[n_vars] uint8,
        wide_idx[cap] uint32, wide_val[cap, 32] uint8."""
        a, b, c, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        rc = self.ctx.L.k16_prover_compact_buffers(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(cap))
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())
        n, k = self.info()["n_vars"], int(cap.value)
        narrow = np.ctypeslib.as_array((C.c_uint8 * n).from_address(a.value))
        idx = np.ctypeslib.as_array((C.c_uint32 * k).from_address(b.value))
        val = np.ctypeslib.as_array((C.c_uint8 * (k * 32)).from_address(c.value)).reshape(k, 32)
        return narrow, idx, val

    def prove_compact(self, n_wide, r=None, s=None):
        """k16_prover_prove_compact: the witness is what compact_buffers() holds."""
        buf = C.create_string_buffer(4096)
        ms = C.c_float()
        R_ = np.frombuffer(bytes(r), dtype=np.uint8).copy() if r is not None else None
        S_ = np.frombuffer(bytes(s), dtype=np.uint8).copy() if s is not None else None
        rc = self.ctx.L.k16_prover_prove_compact(self.h, int(n_wide), _p(R_), _p(S_), buf, 4096, C.byref(ms))
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())
        self.last_device_ms = ms.value
        return buf.value.decode()

    def set_vk(self, vk):
        """k16_prover_set_vk: the VerifyingKey the *_verified calls check against (None detaches).  The prover does not own
        it: keep it alive while it is attached."""
        rc = self.ctx.L.k16_prover_set_vk(self.h, vk.h if vk is not None else None)
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())

    def _verified(self, call, r, s):
        buf = C.create_string_buffer(4096)
        ms = C.c_float()
        R_ = np.frombuffer(bytes(r), dtype=np.uint8).copy() if r is not None else None
        S_ = np.frombuffer(bytes(s), dtype=np.uint8).copy() if s is not None else None
        proof = np.zeros(256, dtype=np.uint8)
        ok = C.c_uint8(0)
        rc = call(_p(R_), _p(S_), buf, 4096, C.byref(ms), _p(proof), C.byref(ok))
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())
        self.last_device_ms = ms.value
        return buf.value.decode(), proof.tobytes(), int(ok.value)

    def prove_mem_verified(self, wtns, r=None, s=None):
        """k16_prover_prove_mem_verified: (json, proof_bytes, ok) -- prove_mem's JSON, the proof as 256 bytes A | B | C in
        VerifyingKey.verify_batch's format, and that call's flag for it with the witness's public inputs."""
        wtns = np.ascontiguousarray(wtns, dtype=np.uint8)
        L, h, n_vars = self.ctx.L, self.h, wtns.size // 32
        return self._verified(lambda *a: L.k16_prover_prove_mem_verified(h, _p(wtns), n_vars, *a), r, s)

    def prove_compact_verified(self, n_wide, r=None, s=None):
        """k16_prover_prove_compact_verified: as prove_mem_verified, for the witness compact_buffers() holds."""
        L, h = self.ctx.L, self.h
        return self._verified(lambda *a: L.k16_prover_prove_compact_verified(h, int(n_wide), *a), r, s)

    def prove_file_verified(self, wtns_path, r=None, s=None):
        """k16_prover_prove_file_verified: as prove_mem_verified, for a .wtns file."""
        L, h, wall = self.ctx.L, self.h, C.c_float()
        path = str(wtns_path).encode()
        return self._verified(lambda R_, S_, buf, cap, ms, proof, ok: L.k16_prover_prove_file_verified(
            h, path, R_, S_, buf, cap, ms, C.byref(wall), proof, ok), r, s)

    def set_r1cs(self, r1cs):
        """k16_prover_set_r1cs: the R1cs every prove call from now on checks its witness against (None detaches).  The prover
        does not own it: keep it alive while it is attached."""
        rc = self.ctx.L.k16_prover_set_r1cs(self.h, r1cs.h if r1cs is not None else None)
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())

    def last_check(self, cap=R1CS_REPORT_MAX):
        """k16_prover_last_check: (status, n_failed, list of the lowest min(n_failed, cap, R1CS_REPORT_MAX) broken constraints)
        of the last prove call; status is one of the CHECK_* values."""
        cap = int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        st, n = C.c_int32(), C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_prover_last_check(self.h, C.byref(st), C.byref(n), _p(out), cap))
        return int(st.value), int(n.value), out[:min(int(n.value), cap, R1CS_REPORT_MAX)].tolist()

    def warmup_status(self):
        return int(self.ctx.L.k16_prover_warmup_status(self.h))

    def last_h(self):
        n = self.info()["domain_size"]
        out = np.zeros((n, 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.L.k16_prover_last_h(self.h, _p(out)))
        return out

    def close(self):
        if self.h:
            self.ctx.L.k16_prover_destroy(self.h)
            self.h = None


class R1cs:
    """A circuit's .r1cs file on the device (k16_r1cs_*): which constraints does a witness break?  path_or_bytes: a file
    name or the file's bytes.  The check methods return (n_failed, ndarray of the lowest min(n_failed, cap) constraint
    numbers, ascending); cap=None asks for all of them."""

    def __init__(self, ctx, path_or_bytes):
        self.ctx = ctx
        h = C.c_void_p()
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            raw = bytes(path_or_bytes)
            rc = ctx.L.k16_r1cs_create_mem(ctx.h, raw, len(raw), C.byref(h))
        else:
            rc = ctx.L.k16_r1cs_create(ctx.h, str(path_or_bytes).encode(), C.byref(h))
        if rc:
            raise K16Error(rc, (ctx.L.k16_last_error(ctx.h) or b"").decode())
        self.h = h

    def info(self):
        nw, npub, m, nt = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_r1cs_info(self.h, C.byref(nw), C.byref(npub), C.byref(m), C.byref(nt)))
        return dict(n_wires=nw.value, n_public=npub.value, n_constraints=m.value, n_terms=nt.value)

    def _check(self, call, cap, err_ctx=None):
        cap = self.info()["n_constraints"] if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        n = C.c_uint64()
        rc = call(C.byref(n), _p(out), cap)
        if rc:
            c = err_ctx or self.ctx
            raise K16Error(rc, (c.L.k16_last_error(c.h) or b"").decode())
        return int(n.value), out[:min(int(n.value), cap)].copy()

    def check(self, wtns, cap=None):
        """k16_r1cs_check_mem: wtns = n_wires x 32 bytes, standard form."""
        wtns = np.ascontiguousarray(wtns, dtype=np.uint8)
        L, c, h = self.ctx.L, self.ctx.h, self.h
        return self._check(lambda *a: L.k16_r1cs_check_mem(c, h, _p(wtns), wtns.size // 32, *a), cap)

    def check_file(self, path, cap=None):
        L, c, h = self.ctx.L, self.ctx.h, self.h
        return self._check(lambda *a: L.k16_r1cs_check_file(c, h, str(path).encode(), *a), cap)

    def check_prover(self, prover, cap=None):
        """k16_r1cs_check_prover_witness: the witness of prover's last prove call, read in place on the device."""
        L, h = self.ctx.L, self.h
        return self._check(lambda *a: L.k16_r1cs_check_prover_witness(prover.h, h, *a), cap, err_ctx=prover.ctx)

    def values(self, i):
        """(A.w, B.w, C.w) of constraint i as the last check computed them, as ints."""
        out = np.zeros(96, dtype=np.uint8)
        self.ctx._chk(self.ctx.L.k16_r1cs_last_values(self.h, int(i), _p(out)))
        return tuple(int.from_bytes(out[32 * k:32 * k + 32].tobytes(), "little") for k in range(3))

    def unbound_wires(self, cap=None, status=False):
        """k16_r1cs_unbound_wires on the sums of the last completed check: (n_absent, n_unbound, wires, classes) with the lowest
        min(n_absent + n_unbound, cap) wires that are not WIRE_BOUND, ascending, and their WIRE_* classes as uint8; cap=None
        asks for all of them.  status=True appends the class of every wire (n_wires x uint8)."""
        n_wires = self.info()["n_wires"]
        cap = n_wires if cap is None else int(cap)
        wires, cls = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint8)
        full = np.zeros(n_wires, dtype=np.uint8) if status else None
        na, nu = C.c_uint64(), C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_r1cs_unbound_wires(self.h, C.byref(na), C.byref(nu), _p(wires), _p(cls), cap,
                                                        _p(full) if status else None))
        k = min(int(na.value) + int(nu.value), cap)
        out = (int(na.value), int(nu.value), wires[:k].copy(), cls[:k].copy())
        return out + (full,) if status else out

    def second_values(self, cap=None, status=False):
        """k16_r1cs_second_values on the sums of the last completed check: (n, wires, shifts) with the lowest min(n, cap) wires
        that are WIRE_TWO_VALUED, ascending, and their shifts as Python ints (wire + shift mod r is the second value); cap=None
        asks for all of them.  status=True appends the class 0 .. 3 of every wire (n_wires x uint8)."""
        n_wires = self.info()["n_wires"]
        cap = n_wires if cap is None else int(cap)
        wires, shifts = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros((max(cap, 1), 32), dtype=np.uint8)
        full = np.zeros(n_wires, dtype=np.uint8) if status else None
        n = C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_r1cs_second_values(self.h, C.byref(n), _p(wires), _p(shifts), cap, _p(full) if status else None))
        k = min(int(n.value), cap)
        out = (int(n.value), wires[:k].copy(), [int.from_bytes(shifts[i].tobytes(), "little") for i in range(k)])
        return out + (full,) if status else out

    def determined_wires(self, seed=None, cap=None, want_maps=False, rules=None):
        """k16_r1cs_determined_wires on the sums of the last completed check: (n_derived, n_absent, n_open, n_rounds, wires) with
        the lowest min(n_open, cap) DET_OPEN wires, ascending; cap=None asks for all of them.  seed: the wires whose values are
        given (wire 0 is added); None: the inputs the .r1cs header names.  want_maps=True appends the class of every wire
        (uint8), its round and its deriving constraint (uint32, DET_NONE where there is none).
        rules: None for k16_r1cs_determined_wires; DET_RULE_PIN or DET_RULE_PIN | DET_RULE_BITS for
        k16_r1cs_determined_wires_ex, whose result gains n_by_bits at the end and, with want_maps, rule (uint8: 0 seed or
        underived, 1 the PIN rule, 2 the bit rule) behind it."""
        n_wires = self.info()["n_wires"]
        cap = n_wires if cap is None else int(cap)
        if cap < 0:
            raise ValueError("cap must not be negative")
        if seed is not None:
            seed = [int(s) for s in seed]
            if any(s < 0 or s > 0xFFFFFFFF for s in seed):
                raise ValueError("a seed wire is no 32-bit number")
            n_seed, seed = len(seed), np.array(seed or [0], dtype=np.uint32)     # (an empty list is no NULL)
        wires = np.zeros(max(cap, 1), dtype=np.uint32)
        status = np.zeros(n_wires, dtype=np.uint8) if want_maps else None
        rounds, by = (np.zeros(n_wires, dtype=np.uint32) for _ in range(2)) if want_maps else (None, None)
        nd, na, no, nr = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        head = (self.h, _p(seed) if seed is not None else None, 0 if seed is None else n_seed)
        common = (C.byref(nd), C.byref(na), C.byref(no), C.byref(nr), _p(wires), cap,
                  *((_p(status), _p(rounds), _p(by)) if want_maps else (None, None, None)))
        if rules is None:
            self.ctx._chk(self.ctx.L.k16_r1cs_determined_wires(*head, *common))
        else:
            nb = C.c_uint64()
            rule = np.zeros(n_wires, dtype=np.uint8) if want_maps else None
            self.ctx._chk(self.ctx.L.k16_r1cs_determined_wires_ex(*head, int(rules), *common, C.byref(nb), _p(rule) if want_maps else None))
        out = (int(nd.value), int(na.value), int(no.value), int(nr.value), wires[:min(int(no.value), cap)].copy())
        if want_maps:
            out += (status, rounds, by)
        if rules is not None:
            out += (int(nb.value),) + ((rule,) if want_maps else ())
        return out

    def held_wires(self, mark=False):
        """k16_r1cs_held_wires: the number of wires HELD under the last completed check -- some constraint that marks the wire
        BOOLEAN was not found broken; mark=True: (n, ndarray of n_wires uint8, 1 for such a wire)."""
        n = C.c_uint64()
        full = np.zeros(self.info()["n_wires"], dtype=np.uint8) if mark else None
        self.ctx._chk(self.ctx.L.k16_r1cs_held_wires(self.h, C.byref(n), _p(full) if mark else None))
        return (int(n.value), full) if mark else int(n.value)

    def _fixed_mask(self, fixed):
        """n_wires bytes.  THE RULE: a numpy array of dtype uint8 or bool with exactly n_wires elements is a MASK (non-zero = fixed);
        anything else -- a list, a tuple, a set, an array of any other dtype or length -- is a LIST OF WIRES.  To pass a list of
        wires that happens to have n_wires elements, give it as a Python list or as an array of a wider integer type."""
        n_wires = self.info()["n_wires"]
        if isinstance(fixed, np.ndarray) and fixed.size == n_wires and fixed.dtype in (np.uint8, np.bool_):
            return np.ascontiguousarray(fixed != 0, dtype=np.uint8)
        mask = np.zeros(n_wires, dtype=np.uint8)
        idx = np.array([int(s) for s in fixed], dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= n_wires):
            raise ValueError("a fixed wire is out of range")
        mask[idx] = 1
        return mask

    def open_system(self, fixed, cap=None, want_maps=False, max_wires=None):
        """k16_r1cs_open_system on the sums of the last completed check.  fixed: the wires held fixed -- a numpy array of
        dtype uint8 or bool with exactly n_wires elements is read as a mask (non-zero = fixed), anything else as a list of wires;
        wire 0 always is fixed.  Returns a dict: n_forced, n_free, n_undecided, n_skipped, n_absent,
        n_components, n_dims, and wires / classes -- the lowest min(cap, ...) wires that are neither OPEN_FIXED nor OPEN_ABSENT,
        ascending, with their OPEN_* class (cap=None asks for all).  want_maps=True adds status (the class of every wire,
        uint8) and comp (the lowest wire of each wire's component, uint32, OPEN_NO_COMPONENT where there is none).
        max_wires=None is k16_r1cs_open_system itself; a number, OPEN_MAX_WIRES .. OPEN_MAX_WIRES_EX, goes to
        k16_r1cs_open_system_ex: components of up to that many wires are eliminated, larger ones are OPEN_SKIPPED."""
        n_wires = self.info()["n_wires"]
        cap = n_wires if cap is None else int(cap)
        if cap < 0:
            raise ValueError("cap must not be negative")
        mask = self._fixed_mask(fixed)
        wires, cls = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint8)
        status = np.zeros(n_wires, dtype=np.uint8) if want_maps else None
        comp = np.zeros(n_wires, dtype=np.uint32) if want_maps else None
        names = ("n_forced", "n_free", "n_undecided", "n_skipped", "n_absent", "n_components", "n_dims")
        counts = [C.c_uint64() for _ in names]
        tail = [*(C.byref(c) for c in counts), _p(wires), _p(cls), cap, _p(status) if want_maps else None, _p(comp) if want_maps else None]
        if max_wires is None:
            self.ctx._chk(self.ctx.L.k16_r1cs_open_system(self.h, _p(mask), *tail))
        else:
            self.ctx._chk(self.ctx.L.k16_r1cs_open_system_ex(self.h, _p(mask), _max_wires(max_wires), *tail))
        out = {k: int(c.value) for k, c in zip(names, counts)}
        k = min(cap, out["n_forced"] + out["n_free"] + out["n_undecided"] + out["n_skipped"])
        out.update(wires=wires[:k].copy(), classes=cls[:k].copy())
        if want_maps:
            out.update(status=status, comp=comp)
        return out

    def open_direction(self, fixed, wire, max_wires=None):
        """k16_r1cs_open_direction: a dict with the wire's OPEN_* class (cls), its component's wires, LINEAR rows and CROSS
        constraints (comp_wires, comp_rows, comp_cross), the rank, and d: {wire: value} of the canonical direction -- empty
        unless the wire is OPEN_FREE.  Adding d to the witness leaves every unbroken constraint satisfied.  max_wires=None is
        k16_r1cs_open_direction itself; a number goes to k16_r1cs_open_direction_ex, with buffers of that many entries."""
        mask = self._fixed_mask(fixed)
        cls, n = C.c_uint8(), C.c_uint64()
        nums = [C.c_uint32() for _ in range(4)]
        width = OPEN_MAX_WIRES if max_wires is None else max(1, min(_max_wires(max_wires), OPEN_MAX_WIRES_EX))
        wires, vals = np.zeros(width, dtype=np.uint32), np.zeros((width, 32), dtype=np.uint8)
        tail = [int(wire), C.byref(cls), *(C.byref(x) for x in nums), C.byref(n), _p(wires), _p(vals), width]
        if max_wires is None:
            self.ctx._chk(self.ctx.L.k16_r1cs_open_direction(self.h, _p(mask), *tail))
        else:
            self.ctx._chk(self.ctx.L.k16_r1cs_open_direction_ex(self.h, _p(mask), _max_wires(max_wires), *tail))
        d = {int(wires[i]): int.from_bytes(vals[i].tobytes(), "little") for i in range(min(int(n.value), width))}
        return dict(cls=int(cls.value), comp_wires=nums[0].value, comp_rows=nums[1].value, comp_cross=nums[2].value,
                    rank=nums[3].value, d=d)

    def audit(self, seed=None, rules=None, max_passes=64, max_wires=None):
        """The closure and the open-set solve in turns, until the solve forces nothing more: each pass runs the closure
        (determined_wires with `rules`) on the seed, holds fixed what is not DET_OPEN, runs open_system, and adds the FORCED wires
        to the seed -- they are forced given the fixed ones, so the next closure may start from them.  Returns (classes, forced_in,
        passes): the OPEN_* class of every wire after the last pass (a wire forced in an earlier pass is OPEN_FIXED there),
        the pass (1, 2, ...) in which open_system forced each wire (0: never), and the number of passes.  max_wires: the cap
        of open_system (None: k16_r1cs_open_system's own 64)."""
        n_wires = self.info()["n_wires"]
        forced_in = np.zeros(n_wires, dtype=np.uint32)
        for n_pass in range(1, int(max_passes) + 1):
            status = self.determined_wires(seed, cap=0, want_maps=True, rules=rules)[5]
            if seed is None:                                     # the closure's default seed: what this run called DET_SEED
                seed = np.nonzero(status == DET_SEED)[0].tolist()
            res = self.open_system(status != DET_OPEN, cap=0, want_maps=True, max_wires=max_wires)
            forced = np.nonzero(res["status"] == OPEN_FORCED)[0]
            if forced.size == 0:
                return res["status"], forced_in, n_pass
            forced_in[forced] = n_pass
            seed = sorted({int(x) for x in seed} | set(forced.tolist()))
        raise RuntimeError("audit: open_system still forces wires after %d passes" % max_passes)

    def boolean_wires(self, mark=False):
        """k16_r1cs_boolean_wires: the number of wires some constraint of the circuit holds to {0, 1}; mark=True: (n, ndarray of
        n_wires uint8, 1 for such a wire).  Needs no check."""
        n = C.c_uint64()
        full = np.zeros(self.info()["n_wires"], dtype=np.uint8) if mark else None
        self.ctx._chk(self.ctx.L.k16_r1cs_boolean_wires(self.h, C.byref(n), _p(full) if mark else None))
        return (int(n.value), full) if mark else int(n.value)

    def complete_witness(self, wtns, given=None, cap=None, cap_failed=None, want_maps=False, rules=None, cap_infeasible=None):
        """k16_r1cs_complete_witness: the values the given wires force.  wtns: n_wires x 32 bytes, standard form; only the given
        positions (and wire 0 = 1) are read.  given: the wires whose values are given (wire 0 is added); None: the inputs the
        .r1cs header names.  Returns a dict: wtns (a new uint8 array: givens kept, solved values filled in, every other wire 0),
        n_solved, n_absent, n_open, n_rounds, n_failed, n_open_constraints, failed (the lowest min(n_failed, cap_failed) broken
        closed constraints, ascending), wires (the lowest min(n_open, cap) SOLVE_OPEN wires, ascending); None for a cap asks for
        all.  want_maps=True adds status (uint8), round and by (uint32, DET_NONE where there is none) of every wire.  The
        object is left as check(result["wtns"]) would leave it.
        rules: None for k16_r1cs_complete_witness; SOLVE_RULE_LINEAR or SOLVE_RULE_LINEAR | SOLVE_RULE_BITS for
        k16_r1cs_complete_witness_ex, which adds n_by_bits, n_infeasible, infeasible (the lowest min(n_infeasible, cap_infeasible)
        infeasible bit rows of the final state, ascending) and, with want_maps, rule (uint8: 0 none or given, 1 linear, 2 bits)."""
        info = self.info()
        n_wires = info["n_wires"]
        cap = n_wires if cap is None else int(cap)
        cap_failed = info["n_constraints"] if cap_failed is None else int(cap_failed)
        if cap < 0 or cap_failed < 0:
            raise ValueError("a cap must not be negative")
        out = np.array(np.frombuffer(wtns, dtype=np.uint8) if isinstance(wtns, (bytes, bytearray, memoryview)) else wtns,
                       dtype=np.uint8).reshape(-1)
        if out.size != n_wires * 32:
            raise ValueError("wtns does not hold n_wires x 32 bytes")
        if given is not None:
            given = [int(s) for s in given]
            if any(s < 0 or s > 0xFFFFFFFF for s in given):
                raise ValueError("a given wire is no 32-bit number")
            n_given, given = len(given), np.array(given or [0], dtype=np.uint32)  # (an empty list is no NULL)
        wires, failed = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap_failed, 1), dtype=np.uint32)
        status = np.zeros(n_wires, dtype=np.uint8) if want_maps else None
        rounds, by = (np.zeros(n_wires, dtype=np.uint32) for _ in range(2)) if want_maps else (None, None)
        ns, na, no, nf, noc, nr = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        head = (self.h, _p(out), _p(given) if given is not None else None, 0 if given is None else n_given)
        common = (C.byref(ns), C.byref(na), C.byref(no), C.byref(nr), C.byref(nf), _p(failed), cap_failed, C.byref(noc), _p(wires), cap,
                  *((_p(status), _p(rounds), _p(by)) if want_maps else (None, None, None)))
        if rules is None:
            self.ctx._chk(self.ctx.L.k16_r1cs_complete_witness(*head, *common))
        else:
            cap_infeasible = info["n_constraints"] if cap_infeasible is None else int(cap_infeasible)
            if cap_infeasible < 0:
                raise ValueError("a cap must not be negative")
            infeasible = np.zeros(max(cap_infeasible, 1), dtype=np.uint32)
            rule = np.zeros(n_wires, dtype=np.uint8) if want_maps else None
            nb, ni = C.c_uint64(), C.c_uint64()
            self.ctx._chk(self.ctx.L.k16_r1cs_complete_witness_ex(*head, int(rules), *common, C.byref(nb), C.byref(ni), _p(infeasible),
                                                                 cap_infeasible, _p(rule) if want_maps else None))
        res = dict(wtns=out, n_solved=int(ns.value), n_absent=int(na.value), n_open=int(no.value), n_rounds=int(nr.value),
                   n_failed=int(nf.value), n_open_constraints=int(noc.value), failed=failed[:min(int(nf.value), cap_failed)].copy(),
                   wires=wires[:min(int(no.value), cap)].copy())
        if want_maps:
            res.update(status=status, round=rounds, by=by)
        if rules is not None:
            res.update(n_by_bits=int(nb.value), n_infeasible=int(ni.value),
                       infeasible=infeasible[:min(int(ni.value), cap_infeasible)].copy())
            if want_maps:
                res.update(rule=rule)
        return res

    def wire_constraints(self, wire, cap=None):
        """k16_r1cs_wire_constraints: (n, ndarray of the lowest min(n, cap) constraints the wire has a non-zero merged
        coefficient in, ascending); cap=None asks for all of them.  Host only."""
        cap = self.info()["n_constraints"] if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        n = C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_r1cs_wire_constraints(self.h, int(wire), C.byref(n), _p(out), cap))
        return int(n.value), out[:min(int(n.value), cap)].copy()

    def incidences(self):
        """k16_r1cs_incidences: the number of (wire, constraint) pairs with a non-zero merged coefficient."""
        n = C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_r1cs_incidences(self.h, C.byref(n)))
        return int(n.value)

    def match_zkey(self, zkey_bytes):
        """k16_r1cs_match_zkey: 0 when the zkey was made from this circuit, else 1 header / 2 A / 3 B / 4 public rows
        (details: last_error())."""
        zkey_bytes = bytes(zkey_bytes)
        mm = C.c_uint32()
        self.ctx._chk(self.ctx.L.k16_r1cs_match_zkey(self.ctx.h, self.h, zkey_bytes, len(zkey_bytes), C.byref(mm)))
        return int(mm.value)

    def setup_size(self):
        """k16_r1cs_setup_size: the exact size in bytes of the key setup() makes."""
        n = C.c_uint64()
        self.ctx._chk(self.ctx.L.k16_r1cs_setup_size(self.h, C.byref(n)))
        return int(n.value)

    @staticmethod
    def _trapdoor(trapdoor):
        if trapdoor is None:
            return None
        if isinstance(trapdoor, (bytes, bytearray)):
            assert len(trapdoor) == 160
            return bytes(trapdoor)
        assert len(trapdoor) == 5
        return b"".join(int(x).to_bytes(32, "little") for x in trapdoor)

    def setup(self, trapdoor=None, ctx=None):
        """k16_r1cs_setup: a Groth16 zkey for this circuit as bytes.  trapdoor: (tau, alpha, beta, gamma, delta) as ints in [1, r)
        or 160 bytes; None draws them from the OS.  DEVELOPMENT AND TEST MATERIAL: whoever holds the trapdoor can forge proofs."""
        ctx = ctx or self.ctx
        out = np.empty(self.setup_size(), dtype=np.uint8)
        n = C.c_size_t()
        ctx._chk(ctx.L.k16_r1cs_setup(ctx.h, self.h, self._trapdoor(trapdoor), _p(out), out.size, C.byref(n)))
        assert n.value == out.size
        return out.tobytes()

    def setup_file(self, path, trapdoor=None):
        """k16_r1cs_setup_file: the same key, written to path."""
        self.ctx._chk(self.ctx.L.k16_r1cs_setup_file(self.ctx.h, self.h, self._trapdoor(trapdoor), str(path).encode()))

    def last_error(self):
        return (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode()

    def close(self):
        if self.h:
            self.ctx.L.k16_r1cs_destroy(self.h)
            self.h = None


def generator_mul_info(group):
    """k16_generator_mul_info: (window bits, number of windows) of a group's generator table."""
    w, nw = C.c_uint(), C.c_uint()
    rc = load().k16_generator_mul_info(group, C.byref(w), C.byref(nw))
    if rc:
        raise K16Error(rc)
    return int(w.value), int(nw.value)


def _zkey_n_public(head):
    """nPublic from the start of an iden3 zkey (section 2 of a Groth16 key: n8q, q, n8r, r, nVars, nPublic, ...)."""
    nsec = int.from_bytes(head[8:12], "little")
    pos = 12
    for _ in range(nsec):
        if pos + 12 > len(head):
            break
        typ, size = int.from_bytes(head[pos:pos + 4], "little"), int.from_bytes(head[pos + 4:pos + 12], "little")
        if typ == 2:
            o = pos + 12 + 4 + 32 + 4 + 32 + 4
            return int.from_bytes(head[o:o + 4], "little")
        pos += 12 + size
    raise ValueError("zkey: section 2 not within the first %d bytes" % len(head))


class VerifyingKey:
    """Groth16 verifying key resident on the GPU (k16_vk_create) + batched verification (k16_verify_batch): the mirror of
    the service's prepared_vk / verify_proof pair (prover-service/src/request_handler/types.rs:141-196,
    prover_handler.rs:329-336).  vk: dict(alpha1, beta2, gamma2, delta2, ic=[...]) of affine Montgomery bytes."""

    def __init__(self, ctx, vk):
        self.ctx, self.n_ic = ctx, len(vk["ic"])
        h = C.c_void_p()
        b = lambda x: np.frombuffer(bytes(x), dtype=np.uint8).copy()
        ic = b(b"".join(vk["ic"]))
        ctx._chk(ctx.L.k16_vk_create(ctx.h, _p(b(vk["alpha1"])), _p(b(vk["beta2"])), _p(b(vk["gamma2"])), _p(b(vk["delta2"])),
                                     _p(ic), self.n_ic, C.byref(h)))
        self.h = h

    @classmethod
    def from_zkey(cls, ctx, path_or_bytes):
        """The key a proving key carries (k16_vk_create_from_zkey[_file]): alpha1, beta2, gamma2, delta2 of section 2 and IC
        of section 3.  path_or_bytes: a file name, or the zkey's bytes."""
        self = cls.__new__(cls)
        self.ctx = ctx
        h = C.c_void_p()
        if isinstance(path_or_bytes, str):
            rc = ctx.L.k16_vk_create_from_zkey_file(ctx.h, path_or_bytes.encode(), C.byref(h))
            with open(path_or_bytes, "rb") as f:
                head = f.read(4096)
        else:
            z = np.frombuffer(bytes(path_or_bytes), dtype=np.uint8).copy()
            rc = ctx.L.k16_vk_create_from_zkey(ctx.h, _p(z), z.size, C.byref(h))
            head = bytes(path_or_bytes[:4096])
        if rc:
            raise K16Error(rc, (ctx.L.k16_last_error(ctx.h) or b"").decode())
        self.h = h
        self.n_ic = _zkey_n_public(head) + 1
        return self

    def split_gt(self, proofs, inputs):
        """k16_verify_split_gt (n <= 64): the split check's two values per proof -- (early, gt), each (n, 384) uint8: the
        multi-Miller value of (A,B), (vk_x,-gamma) before any final exponentiation, and the GT value coop_gt also gives.
        Raises K16Error(ARG) for a proof that fails the point checks, has a zero point, or whose vk_x is infinity."""
        n = len(proofs)
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8).copy()
        inp = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for row in inputs for x in row), dtype=np.uint8).copy()
        early = np.zeros((n, 384), dtype=np.uint8)
        gt = np.zeros((n, 384), dtype=np.uint8)
        rc = self.ctx.L.k16_verify_split_gt(self.ctx.h, self.h, _p(pr), _p(inp) if inp.size else None, n, _p(early), _p(gt))
        if rc < 0:
            raise K16Error(rc, (self.ctx.L.k16_last_error(self.ctx.h) or b"").decode())
        return early, gt

    def verify_batch(self, proofs, inputs):
        """proofs: list of 256-byte A | B | C; inputs: per proof a list of n_ic - 1 ints.  Returns a list of bools."""
        n = len(proofs)
        if n == 0:
            return []
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8).copy()
        assert pr.size == 256 * n
        inp = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for row in inputs for x in row), dtype=np.uint8).copy()
        assert inp.size == n * (self.n_ic - 1) * 32
        ok = np.zeros(n, dtype=np.uint8)
        self.ctx._chk(self.ctx.L.k16_verify_batch(self.ctx.h, self.h, _p(pr), _p(inp) if inp.size else None, n, _p(ok)))
        return [bool(v) for v in ok]

    def verify_batch_checked(self, proofs, inputs):
        """k16_verify_batch_checked: verify_batch plus the G2 subgroup test of every B.  Returns (flags, reasons): lists of
        bools and of ints (0 accepted, 1..3 the first failing point's PT_* status, A then B then C, 4 pairing mismatch)."""
        n = len(proofs)
        if n == 0:
            return [], []
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8).copy()
        assert pr.size == 256 * n
        inp = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for row in inputs for x in row), dtype=np.uint8).copy()
        assert inp.size == n * (self.n_ic - 1) * 32
        ok = np.zeros(n, dtype=np.uint8)
        why = np.zeros(n, dtype=np.uint8)
        self.ctx._chk(self.ctx.L.k16_verify_batch_checked(self.ctx.h, self.h, _p(pr), _p(inp) if inp.size else None, n,
                                                          _p(ok), _p(why)))
        return [bool(v) for v in ok], [int(v) for v in why]

    def verify_batch_folded(self, proofs, inputs):
        """k16_verify_batch_folded: the small-exponent batch test -- one final exponentiation for the whole batch, random
        128-bit weights drawn by the library.  Same flags and reasons as verify_batch_checked (a wrong proof slips through
        with probability ~2^-128).  Returns (flags, reasons, folded): folded is True when the fold itself decided the
        batch, False when the call went through the per-proof path (batch below VERIFY_FOLD_MIN, or a wrong proof in it)."""
        n = len(proofs)
        if n == 0:
            return [], [], False
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8).copy()
        assert pr.size == 256 * n
        inp = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for row in inputs for x in row), dtype=np.uint8).copy()
        assert inp.size == n * (self.n_ic - 1) * 32
        ok = np.zeros(n, dtype=np.uint8)
        why = np.zeros(n, dtype=np.uint8)
        folded = C.c_uint8(0)
        self.ctx._chk(self.ctx.L.k16_verify_batch_folded(self.ctx.h, self.h, _p(pr), _p(inp) if inp.size else None, n,
                                                         _p(ok), _p(why), C.byref(folded)))
        return [bool(v) for v in ok], [int(v) for v in why], bool(folded.value)

    def fold_gt(self, proofs, inputs, weights):
        """The value of the fold's left-hand side after the final exponentiation under the caller's weights (ints below
        2^128; zero drops the proof), k16_verify_fold_gt: 384 bytes in the format of Context.pairing_vec.  Raises
        K16Error(ARG) when a proof fails the point checks or has a zero point."""
        n = len(proofs)
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8).copy()
        assert pr.size == 256 * n and len(weights) == n
        inp = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for row in inputs for x in row), dtype=np.uint8).copy()
        assert inp.size == n * (self.n_ic - 1) * 32
        w = np.frombuffer(b"".join(int(x).to_bytes(16, "little") for x in weights), dtype=np.uint8).copy()
        out = np.zeros(384, dtype=np.uint8)
        self.ctx._chk(self.ctx.L.k16_verify_fold_gt(self.ctx.h, self.h, _p(pr), _p(inp) if inp.size else None, n, _p(w), _p(out)))
        return out.tobytes()

    def coop_gt(self, proofs, inputs):
        """The GT value e(A,B) e(vk_x,-gamma) e(C,-delta) of every proof as the wave-cooperative path computes it
        (k16_verify_coop_gt): (n, 384) uint8.  Raises K16Error(ARG) when that path does not apply."""
        n = len(proofs)
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8).copy()
        inp = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for row in inputs for x in row), dtype=np.uint8).copy()
        out = np.zeros((n, 384), dtype=np.uint8)
        self.ctx._chk(self.ctx.L.k16_verify_coop_gt(self.ctx.h, self.h, _p(pr), _p(inp) if inp.size else None, n, _p(out)))
        return out

    def close(self):
        if self.h:
            self.ctx.L.k16_vk_destroy(self.h)
            self.h = None


PT_OK, PT_NONCANONICAL, PT_OFF_CURVE, PT_NOT_IN_SUBGROUP = 0, 1, 2, 3     # include/k16.h K16_PT_*
VERIFY_PAIRING_MISMATCH = 4
VERIFY_FOLD_MIN = 2049                                                     # include/k16.h K16_VERIFY_FOLD_MIN


def zkey_check(ctx, zkey):
    """Every point of a Groth16 zkey checked on the GPU (k16_zkey_check / _file).  zkey: bytes-like, or a path.
    Returns dict(ok, n_bad, section, index, status): the first failure in (section, index) order when n_bad > 0."""
    sec, idx, st, nb = C.c_uint32(), C.c_uint64(), C.c_uint8(), C.c_uint64()
    if isinstance(zkey, (str, os.PathLike)):
        rc = ctx.L.k16_zkey_check_file(ctx.h, os.fsencode(zkey), C.byref(sec), C.byref(idx), C.byref(st), C.byref(nb))
    else:
        a = np.frombuffer(zkey, dtype=np.uint8)
        rc = ctx.L.k16_zkey_check(ctx.h, _p(a), a.size, C.byref(sec), C.byref(idx), C.byref(st), C.byref(nb))
    ctx._chk(rc)
    return dict(ok=nb.value == 0, n_bad=nb.value, section=sec.value, index=idx.value, status=st.value)


def pairing_vec(ctx, g1, g2):
    """e(P_i, Q_i) for affine Montgomery G1 (n, 64) / G2 (n, 128) arrays -> (n, 384) uint8 (k16_pairing_vec)."""
    g1 = np.ascontiguousarray(g1, dtype=np.uint8)
    g2 = np.ascontiguousarray(g2, dtype=np.uint8)
    n = g1.shape[0]
    out = np.zeros((n, 384), dtype=np.uint8)
    ctx._chk(ctx.L.k16_pairing_vec(ctx.h, _p(g1), _p(g2), n, _p(out)))
    return out


class ShardedMsm:
    """One MSM sharded over several devices from ONE process (include/k16.h: k16_msm_sharded_*): a context per entry of
    `devices` (entries may repeat), contiguous shards, host-side EC-add fold of the per-shard partial results."""

    def __init__(self, devices, group, n):
        self.L = load()
        self.group, self.n = group, n
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.L.k16_msm_sharded_create(arr, len(devices), group, n, C.byref(h))
        if rc:
            raise K16Error(rc, "k16_msm_sharded_create")
        self.h = h

    def _chk(self, rc):
        if rc:
            raise K16Error(rc, (self.L.k16_msm_sharded_last_error(self.h) or b"").decode())

    def count(self):
        return self.L.k16_msm_sharded_count(self.h)

    def shard_range(self, r):
        lo, hi = C.c_uint64(), C.c_uint64()
        self._chk(self.L.k16_msm_sharded_range(self.h, r, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def shard_ctx(self, r):
        """A borrowed Context over shard r's k16_ctx (owned by the ShardedMsm: do not close it)."""
        c = Context.__new__(Context)
        c.L, c.h, c.borrowed = self.L, C.c_void_p(self.L.k16_msm_sharded_ctx(self.h, r)), True
        c.device = -1
        return c

    def set_bases(self, h_bases):
        h_bases = np.ascontiguousarray(h_bases)
        assert h_bases.nbytes == self.n * AFF_BYTES[self.group]
        self._chk(self.L.k16_msm_sharded_set_bases(self.h, _p(h_bases)))

    def set_bases_device(self, r, d_slice):
        self._chk(self.L.k16_msm_sharded_set_bases_device(self.h, r, d_slice.ptr if d_slice is not None else None))

    def run(self, h_scalars):
        h_scalars = np.ascontiguousarray(h_scalars)
        assert h_scalars.nbytes == self.n * 32
        x = np.zeros(XYZZ_BYTES[self.group], dtype=np.uint8)
        a = np.zeros(AFF_BYTES[self.group], dtype=np.uint8)
        self._chk(self.L.k16_msm_sharded_run(self.h, _p(h_scalars), _p(x), _p(a)))
        return x.tobytes(), a.tobytes()

    def run_device(self, d_scalars):
        arr = (C.c_void_p * len(d_scalars))(*[d.ptr for d in d_scalars])
        x = np.zeros(XYZZ_BYTES[self.group], dtype=np.uint8)
        a = np.zeros(AFF_BYTES[self.group], dtype=np.uint8)
        self._chk(self.L.k16_msm_sharded_run_device(self.h, arr, _p(x), _p(a)))
        return x.tobytes(), a.tobytes()

    def set_piece_rows(self, host_rows=0, device_rows=0):
        """rows per device pass inside a shard (include/k16.h; 0 = default 2^22 / 2^24); same result for any value"""
        self._chk(self.L.k16_msm_sharded_set_piece_rows(self.h, host_rows, device_rows))

    def last_ms(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self.L.k16_msm_sharded_last_ms(self.h, C.byref(a), C.byref(b), C.byref(c))
        return dict(shards_ms=a.value, fold_ms=b.value, total_ms=c.value)

    def close(self):
        if self.h:
            self.L.k16_msm_sharded_destroy(self.h)
            self.h = None


class RankComm:
    """One process per GPU: the shards' partial results exchanged with ONE ncclAllGather (RCCL, dlopen'ed by the library) and
    folded on every rank (include/k16.h: k16_rank_comm_*).  `unique_id` = the 128 bytes rank 0 got from RankComm.unique_id(),
    handed to the other ranks by the launcher."""

    @staticmethod
    def unique_id():
        L = load()
        buf = np.zeros(128, dtype=np.uint8)
        rc = L.k16_rank_comm_unique_id(_p(buf))
        if rc:
            raise K16Error(rc, (L.k16_rank_comm_load_error() or b"").decode())
        return buf.tobytes()

    def __init__(self, ctx, rank, world, unique_id):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        uid = np.frombuffer(unique_id, dtype=np.uint8).copy()
        ctx._chk(self.L.k16_rank_comm_create(ctx.h, rank, world, _p(uid), C.byref(h)))
        self.h, self.world = h, world

    def allgather_fold(self, group, partial_xyzz):
        part = np.frombuffer(partial_xyzz, dtype=np.uint8).copy()
        x = np.zeros(XYZZ_BYTES[group], dtype=np.uint8)
        a = np.zeros(AFF_BYTES[group], dtype=np.uint8)
        self.ctx._chk(self.L.k16_rank_comm_allgather_fold(self.h, group, _p(part), _p(x), _p(a)))
        return x.tobytes(), a.tobytes()

    def allgather_start(self, group, partial_xyzz):
        """enqueue one exchange and return (include/k16.h: up to 4 in flight, completed in order by allgather_finish)"""
        part = np.frombuffer(partial_xyzz, dtype=np.uint8).copy()
        self.ctx._chk(self.L.k16_rank_comm_allgather_start(self.h, group, _p(part)))
        self._groups = getattr(self, "_groups", []) + [group]

    def allgather_finish(self):
        group = self._groups.pop(0)
        x = np.zeros(XYZZ_BYTES[group], dtype=np.uint8)
        a = np.zeros(AFF_BYTES[group], dtype=np.uint8)
        self.ctx._chk(self.L.k16_rank_comm_allgather_finish(self.h, _p(x), _p(a)))
        return x.tobytes(), a.tobytes()

    def close(self):
        if self.h:
            self.L.k16_rank_comm_destroy(self.h)
            self.h = None
