"""bls-verify-gadget_amd — MI355X-native batched witness generation for the BLS12-381 signature-verify gadget.

Host-side mirror (Python over the C ABI of include/blsw.h) of the reference's gadget surface:
    BlsSignatureVerifyGadget::verify(&ParametersVar, &PublicKeyVar, &[UInt8], &SignatureVar) -> Boolean
        (/root/reference/src/constraints.rs:79-128)
    AllocVar::new_variable(.., mode) for ParametersVar / PublicKeyVar / SignatureVar (constraints.rs:194-249)
The product path is the HIP library only: importing works without a GPU (layout is host logic), but every
compute entry point raises if libblsw.so or a HIP device is missing. Nothing here touches oracle/.
"""
import ctypes
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# BLSW_LIB: an alternative build of the same library (A/B runs of compile-time choices, tools/ab_build.sh); default: the in-tree one
LIB_PATH = os.environ.get("BLSW_LIB") or os.path.join(HERE, "libblsw.so")

FP_BYTES = 48
_LAYOUT_FIELDS = (
    "msg_len n_instance_vars n_witness sha_bits off_msg off_pk_alloc off_sig_alloc off_pk_not_zero off_expand off_map0 off_map1 "
    "off_add off_cofactor off_prep_h off_prep_pk off_prep_sig off_miller off_final_exp off_is_one n_keys off_keys off_bitmap off_count off_agg "
    "n_pairs stride_msg stride_pk_alloc stride_pk_not_zero stride_hash stride_prep_h stride_prep_pk "
    "params_mode off_params_alloc off_prep_g1 pk_mode sig_mode"
).split()


class blsw_layout_t(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in _LAYOUT_FIELDS]


class blsw_engine_options_t(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32)] + [(n, ctypes.c_uint32) for n in "n_keys pairing_mode g2_mode expand_variant expand_store prio_mode place_lds consumer_mode output_form chain_variant n_pairs cofactor_mode params_mode group_ramp latency_mode pk_mode sig_mode msg_mode agg_inputs shared_keys".split()]


class blsw_matrices_info_t(ctypes.Structure):
    _fields_ = [("n_constraints", ctypes.c_uint64), ("n_instance_vars", ctypes.c_uint64), ("n_witness", ctypes.c_uint64), ("nnz", ctypes.c_uint64 * 3)]


class blsw_matrices_t(ctypes.Structure):
    _fields_ = [("row_ptr", ctypes.POINTER(ctypes.c_uint64) * 3), ("col", ctypes.POINTER(ctypes.c_uint32) * 3), ("val", ctypes.POINTER(ctypes.c_uint64) * 3)]


class blsw_compact_layout_t(ctypes.Structure):
    """where the witnesses of a step live in its compact buffer (include/blsw.h, ABI 14)"""
    _fields_ = [(n, ctypes.c_uint64) for n in "n off_staging off_pair total".split()] + \
               [(n, ctypes.c_uint32) for n in "n_witness off_expand sha_bits sha_words split_row staging_rows pair_rows moved_lo moved_len moved_at".split()]


class blsw_compact_layout_multi_t(ctypes.Structure):
    """where the witnesses of a step of the N+1-pair product live in its compact buffer: bit words and pair tiles by pair lane i * n_pairs + j,
    instance tiles, instance rows (include/blsw.h)"""
    _fields_ = [(n, ctypes.c_uint64) for n in "n off_staging off_inst off_pair total".split()] + \
               [(n, ctypes.c_uint32) for n in "n_pairs n_witness sha_bits sha_words off_expand stride_hash rows_p rows_i pair_rows inst_tile_w off_miller reserved".split()] + \
               [(n, ctypes.c_uint32 * 6) for n in "pair_run_row pair_run_off pair_run_stride pair_run_len".split()] + \
               [(n, ctypes.c_uint32 * 2) for n in "inst_run_row inst_run_off inst_run_len".split()]


COMPACT_BIT, COMPACT_TILE, COMPACT_PAIR = 0, 1, 2  # regions of compact_locate
COMPACT_INST = 3  # compact_locate_multi: an instance tile (COMPACT_TILE: a pair tile, COMPACT_PAIR: the instance rows)

ERR_BUSY = 6


class blsw_dst_t(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_uint8 * 255), ("len", ctypes.c_uint8)]


class BlswError(RuntimeError):
    pass


class BlswBusy(BlswError):
    """consumer_mode engines: the call would have to wait for outputs the caller still holds — drain (wait_step / output_consumed)
    and call again (BLSW_ERR_BUSY)."""


_lib = None


def _load_build_module():
    spec = importlib.util.spec_from_file_location("blsw_build", os.path.join(HERE, "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def build(force=False, verbose=False):
    return _load_build_module().build(force=force, verbose=verbose)


def lib():
    """Loads libblsw.so; fails loudly when the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BlswError("libblsw.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.blsw_layout.argtypes = [u32, ctypes.POINTER(blsw_layout_t)]
        L.blsw_engine_workspace_bytes.argtypes = [u64, u32, u32, u32, ctypes.POINTER(u64)]
        L.blsw_engine_create.argtypes = [ctypes.POINTER(vp), u64, u32, u32, u32, vp, u64]
        L.blsw_engine_workspace_bytes_ex.argtypes = [u64, u32, u32, u32, ctypes.POINTER(blsw_engine_options_t), ctypes.POINTER(u64)]
        L.blsw_engine_submit_aggregate.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]
        L.blsw_engine_create_ex.argtypes = [ctypes.POINTER(vp), u64, u32, u32, u32, ctypes.POINTER(blsw_engine_options_t), vp, u64]
        L.blsw_engine_options_default.argtypes = [ctypes.POINTER(blsw_engine_options_t)]
        L.blsw_engine_submitted.argtypes = [vp, ctypes.POINTER(u64)]
        L.blsw_engine_launched.argtypes = [vp, ctypes.POINTER(u64)]
        L.blsw_engine_materialised.argtypes = [vp, ctypes.POINTER(u64)]
        L.blsw_engine_wait_step.argtypes = [vp, u64, vp]
        L.blsw_engine_output_consumed.argtypes = [vp, vp, vp]
        L.blsw_engine_compact_bytes.argtypes = [vp, ctypes.POINTER(u64)]
        L.blsw_engine_submit_compact.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.blsw_engine_expand_compact.argtypes = [vp, vp, vp, u64, vp]
        L.blsw_engine_submit_aggregate_compact.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.blsw_witness_digest.argtypes = [vp, u64, u64, u32, vp, vp]
        L.blsw_matrices_info.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t)]
        L.blsw_matrices_fill.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t), ctypes.POINTER(blsw_matrices_t)]
        L.blsw_matrices_info_params.argtypes = [u32, u32, ctypes.POINTER(blsw_matrices_info_t)]
        L.blsw_matrices_fill_params.argtypes = [u32, u32, ctypes.POINTER(blsw_matrices_info_t), ctypes.POINTER(blsw_matrices_t)]
        L.blsw_layout_params.argtypes = [u32, u32, ctypes.POINTER(blsw_layout_t)]
        L.blsw_layout_inputs.argtypes = [u32, u32, u32, u32, ctypes.POINTER(blsw_layout_t)]
        L.blsw_matrices_info_inputs.argtypes = [u32, u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t)]
        L.blsw_matrices_fill_inputs.argtypes = [u32, u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t), ctypes.POINTER(blsw_matrices_t)]
        L.blsw_layout_aggregate_inputs.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_layout_t)]
        L.blsw_matrices_info_aggregate_inputs.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t)]
        L.blsw_matrices_fill_aggregate_inputs.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t), ctypes.POINTER(blsw_matrices_t)]
        L.blsw_engine_submit_aggregate_io.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]
        L.blsw_layout_multi.argtypes = [u32, u32, ctypes.POINTER(blsw_layout_t)]
        L.blsw_layout_multi_inputs.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_layout_t)]
        L.blsw_matrices_info_multi_inputs.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t)]
        L.blsw_matrices_fill_multi_inputs.argtypes = [u32, u32, u32, ctypes.POINTER(blsw_matrices_info_t), ctypes.POINTER(blsw_matrices_t)]
        L.blsw_engine_submit_multi_io.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, vp]
        L.blsw_engine_workspace_bytes_multi_inputs.argtypes = [u64, u32, u32, u32, ctypes.POINTER(blsw_engine_options_t), u32, ctypes.POINTER(u64)]
        L.blsw_engine_create_multi_inputs.argtypes = [ctypes.POINTER(vp), u64, u32, u32, u32, ctypes.POINTER(blsw_engine_options_t), u32, vp, u64]
        L.blsw_verify_multi_workspace_bytes.argtypes = [u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_verify_multi_batch.argtypes = [vp, vp, u32, u32, vp, u64, vp, u64, vp, vp, u64, vp]
        L.blsw_engine_destroy.argtypes = [vp]
        L.blsw_engine_submit.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp]
        L.blsw_engine_submit_multi.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp]
        L.blsw_engine_submit_io.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, vp]
        L.blsw_engine_submit_multi_compact.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.blsw_engine_submit_bytes.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp]
        L.blsw_engine_flush.argtypes = [vp, vp]
        L.blsw_engine_expand_stats.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_float)]
        L.blsw_hash_to_g2_workspace_bytes.argtypes = [u64, u32, ctypes.POINTER(u64)]
        L.blsw_hash_to_g2_batch.argtypes = [vp, u32, u64, vp, vp, u64, vp]
        L.blsw_layout_aggregate.argtypes = [u32, u32, ctypes.POINTER(blsw_layout_t)]
        L.blsw_aggregate_workspace_bytes.argtypes = [u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_aggregate_verify_batch.argtypes = [vp, vp, u32, vp, vp, u32, u64, vp, u64, vp, vp, vp, u64, vp]
        L.blsw_decode_batch.argtypes = [vp, vp, u64, vp, vp, vp, vp]
        L.blsw_aggregate_points_workspace_bytes.argtypes = [u32, u64, u32, ctypes.POINTER(u64)]
        L.blsw_aggregate_points_batch.argtypes = [u32, vp, u32, u64, vp, vp, vp, u64, vp]
        L.blsw_combine_points_workspace_bytes.argtypes = [u32, u64, u32, ctypes.POINTER(u64)]
        L.blsw_combine_points_batch.argtypes = [u32, vp, vp, vp, u32, u64, vp, vp, vp, vp, u64, vp]
        L.blsw_lagrange_batch.argtypes = [vp, vp, u32, u64, vp, vp, vp]
        L.blsw_recover_points_batch.argtypes = [u32, vp, vp, vp, u32, u64, vp, vp, vp, u64, vp]
        L.blsw_msm_workspace_bytes.argtypes = [u32, u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_msm_points_batch.argtypes = [u32, vp, vp, vp, u32, u64, u32, vp, vp, vp, u64, vp]
        L.blsw_registry_msm_workspace_bytes.argtypes = [u64, u64, u32, ctypes.POINTER(u64)]
        L.blsw_registry_msm_batch.argtypes = [vp, vp, u64, vp, vp, u64, u32, vp, vp, vp, u64, vp]
        L.blsw_sign_batch.argtypes = [vp, vp, u32, u64, vp, vp, vp, vp, vp, vp, u64, vp]
        L.blsw_verify_workspace_bytes.argtypes = [u64, u32, ctypes.POINTER(u64)]
        L.blsw_verify_batch.argtypes = [vp, vp, vp, u32, u64, vp, vp, vp, u64, vp]
        L.blsw_verify_groups_workspace_bytes.argtypes = [u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_verify_groups_batch.argtypes = [vp, vp, vp, u32, u64, vp, u32, vp, vp, vp, u64, vp]
        L.blsw_verify_pairs_workspace_bytes.argtypes = [u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_verify_pairs_batch.argtypes = [vp, vp, u32, u32, vp, vp, u64, vp, vp, vp, vp, u64, vp]
        L.blsw_committee_verify_workspace_bytes.argtypes = [u64, u32, u32, u32, ctypes.POINTER(u64)]
        L.blsw_committee_verify_batch.argtypes = [vp, u32, vp, vp, vp, u32, u64, vp, u32, vp, vp, vp, vp, vp, vp, u64, vp]
        L.blsw_registry_bytes.argtypes = [u32, ctypes.POINTER(u64)]
        L.blsw_registry_create.argtypes = [ctypes.POINTER(vp), u32, ctypes.c_int32, vp, u64]
        L.blsw_registry_append.argtypes = [vp, vp, u32, vp]
        L.blsw_registry_size.argtypes = [vp, ctypes.POINTER(u32)]
        L.blsw_registry_key_status.argtypes = [vp, ctypes.POINTER(vp)]
        L.blsw_registry_destroy.argtypes = [vp]
        L.blsw_registry_verify_workspace_bytes.argtypes = [u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_registry_verify_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, u64, vp, u32, vp, vp, vp, vp, u64, vp]
        L.blsw_microbench.argtypes = [ctypes.c_int, u32, u32, ctypes.POINTER(ctypes.c_double)]
        L.blsw_fill_rate.argtypes = [vp, u64, u32, ctypes.POINTER(ctypes.c_double)]
        mi, mp = ctypes.POINTER(blsw_matrices_info_t), ctypes.POINTER(blsw_matrices_t)
        L.blsw_r1cs_device_bytes.argtypes = [mi, mp, ctypes.POINTER(u64)]
        L.blsw_r1cs_create.argtypes = [ctypes.POINTER(vp), mi, mp, ctypes.c_int32, vp, u64, vp]
        L.blsw_r1cs_destroy.argtypes = [vp]
        L.blsw_r1cs_check.argtypes = [vp, vp, u64, vp, u64, u64, u32, vp, vp, vp]
        L.blsw_r1cs_evaluate.argtypes = [vp, vp, u64, vp, u64, u64, u32, u64, u64, vp, vp, vp, vp]
        cl = ctypes.POINTER(blsw_compact_layout_t)
        L.blsw_compact_layout.argtypes = [u64, u32, ctypes.POINTER(blsw_engine_options_t), cl]
        L.blsw_compact_locate.argtypes = [cl, u32, u64, ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(u32)]
        L.blsw_r1cs_check_compact.argtypes = [vp, cl, vp, vp, u64, vp, vp, vp]
        L.blsw_r1cs_evaluate_compact.argtypes = [vp, cl, vp, vp, u64, u64, u64, vp, vp, vp, vp]
        L.blsw_keyset_bytes.argtypes = [u32, ctypes.POINTER(u64)]
        L.blsw_keyset_create.argtypes = [ctypes.POINTER(vp), vp, u32, u32, ctypes.c_int32, vp, u64, vp]
        L.blsw_keyset_table.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64)]
        L.blsw_keyset_destroy.argtypes = [vp]
        L.blsw_keyset_broadcast_rate.argtypes = [vp, vp, u64, u64, u32, u32, ctypes.POINTER(ctypes.c_double)]
        L.blsw_engine_submit_aggregate_keyset.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]
        L.blsw_engine_submit_aggregate_keyset_compact.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.blsw_engine_expand_compact_keyset.argtypes = [vp, vp, vp, vp, u64, vp]
        L.blsw_compact_layout_keyset.argtypes = [u64, u32, ctypes.POINTER(blsw_engine_options_t), cl, ctypes.POINTER(u32)]
        L.blsw_r1cs_head_rows.argtypes = [ctypes.POINTER(blsw_matrices_info_t), ctypes.POINTER(blsw_matrices_t), u64, ctypes.POINTER(u64)]
        L.blsw_r1cs_handle_head_rows.argtypes = [vp, u64, ctypes.POINTER(u64)]
        L.blsw_r1cs_check_keyset.argtypes = [vp, vp, vp, vp, vp]
        L.blsw_r1cs_check_compact_keyset.argtypes = [vp, cl, vp, vp, u32, vp, u64, vp, vp, vp]
        L.blsw_r1cs_evaluate_compact_keyset.argtypes = [vp, cl, vp, vp, vp, u64, u64, u64, vp, vp, vp, vp]
        cm = ctypes.POINTER(blsw_compact_layout_multi_t)
        L.blsw_compact_layout_multi.argtypes = [u64, u32, ctypes.POINTER(blsw_engine_options_t), u32, cm]
        L.blsw_compact_locate_multi.argtypes = [cm, u32, u64, ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(u32)]
        L.blsw_compact_locate_multi_range.argtypes = [cm, u32, u32, u64, vp, vp, vp]
        L.blsw_r1cs_pair_families.argtypes = [mi, mp, cm, u64, vp, vp, ctypes.POINTER(u64)]
        L.blsw_r1cs_handle_pair_families.argtypes = [vp, cm, u64, vp, vp, ctypes.POINTER(u64)]
        L.blsw_r1cs_check_compact_multi.argtypes = [vp, cm, vp, vp, u64, vp, vp, vp]
        L.blsw_r1cs_check_compact_multi_ex.argtypes = [vp, cm, vp, vp, u64, u32, vp, vp, vp]
        L.blsw_r1cs_evaluate_compact_multi.argtypes = [vp, cm, vp, vp, u64, u64, u64, vp, vp, vp, vp]
        dp = ctypes.POINTER(blsw_dst_t)
        L.blsw_dst_set.argtypes = [dp, vp, u32]
        L.blsw_dst_default.argtypes = [dp]
        L.blsw_dst_pop.argtypes = [dp]
        L.blsw_hash_to_field_batch.argtypes = [vp, u32, u64, dp, vp, vp]
        for name in _DST_ENTRIES:  # the plain entry's arguments with the tag in front of the stream
            plain = getattr(L, name).argtypes
            getattr(L, name + "_dst").argtypes = list(plain[:-1]) + [dp, plain[-1]]
        L.blsw_pop_prove_batch.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp]
        L.blsw_pop_verify_batch.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp]
        L.blsw_verify_groups_shared_workspace_bytes.argtypes = [u64, u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_verify_groups_shared_batch.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, u32, dp, vp, vp, vp, vp, u64, vp]
        L.blsw_registry_verify_shared_workspace_bytes.argtypes = [u64, u64, u32, u32, ctypes.POINTER(u64)]
        L.blsw_registry_verify_shared_batch.argtypes = [vp, vp, u64, vp, vp, vp, u32, u64, vp, u64, vp, u32, dp, vp, vp, vp, vp, vp, u64, vp]
        _lib = L
    return _lib


_DST_ENTRIES = ["blsw_hash_to_g2_batch", "blsw_sign_batch", "blsw_verify_batch", "blsw_verify_groups_batch", "blsw_verify_pairs_batch", "blsw_committee_verify_batch",
                "blsw_registry_verify_batch"]


EXPORTED_SYMBOLS = ["blsw_version", "blsw_layout", "blsw_engine_options_default", "blsw_engine_workspace_bytes", "blsw_engine_workspace_bytes_ex", "blsw_engine_create",
                    "blsw_engine_create_ex", "blsw_engine_destroy", "blsw_engine_submit", "blsw_engine_submit_bytes", "blsw_engine_submit_multi", "blsw_engine_submit_multi_compact", "blsw_engine_submit_aggregate", "blsw_engine_flush", "blsw_engine_submitted", "blsw_engine_launched", "blsw_engine_materialised", "blsw_engine_wait_step",
                    "blsw_engine_output_consumed", "blsw_engine_compact_bytes", "blsw_engine_submit_compact", "blsw_engine_submit_aggregate_compact", "blsw_engine_expand_compact", "blsw_engine_expand_stats", "blsw_witness_digest", "blsw_hash_to_g2_workspace_bytes", "blsw_hash_to_g2_batch",
                    "blsw_decode_batch", "blsw_layout_aggregate", "blsw_aggregate_workspace_bytes", "blsw_aggregate_verify_batch", "blsw_layout_multi",
                    "blsw_verify_multi_workspace_bytes", "blsw_verify_multi_batch", "blsw_matrices_info", "blsw_matrices_fill", "blsw_sign_batch", "blsw_microbench", "blsw_fill_rate", "blsw_layout_io", "blsw_engine_submit_io", "blsw_verify_workspace_bytes", "blsw_verify_batch", "blsw_verify_groups_workspace_bytes", "blsw_verify_groups_batch", "blsw_committee_verify_workspace_bytes", "blsw_committee_verify_batch", "blsw_matrices_info_io", "blsw_matrices_fill_io",
                    "blsw_layout_params", "blsw_matrices_info_params", "blsw_matrices_fill_params", "blsw_aggregate_points_workspace_bytes", "blsw_aggregate_points_batch",
                    "blsw_r1cs_device_bytes", "blsw_r1cs_create", "blsw_r1cs_destroy", "blsw_r1cs_check", "blsw_r1cs_evaluate", "blsw_layout_inputs",
                    "blsw_matrices_info_inputs", "blsw_matrices_fill_inputs", "blsw_layout_aggregate_inputs", "blsw_matrices_info_aggregate_inputs",
                    "blsw_matrices_fill_aggregate_inputs", "blsw_engine_submit_aggregate_io", "blsw_compact_layout", "blsw_compact_locate",
                    "blsw_r1cs_check_compact", "blsw_r1cs_evaluate_compact", "blsw_keyset_bytes", "blsw_keyset_create", "blsw_keyset_table", "blsw_keyset_destroy",
                    "blsw_keyset_broadcast_rate", "blsw_engine_submit_aggregate_keyset", "blsw_engine_submit_aggregate_keyset_compact",
                    "blsw_engine_expand_compact_keyset", "blsw_compact_layout_keyset", "blsw_r1cs_head_rows", "blsw_r1cs_handle_head_rows", "blsw_r1cs_check_keyset",
                    "blsw_r1cs_check_compact_keyset", "blsw_r1cs_evaluate_compact_keyset", "blsw_layout_multi_inputs", "blsw_matrices_info_multi_inputs",
                    "blsw_matrices_fill_multi_inputs", "blsw_engine_submit_multi_io", "blsw_engine_workspace_bytes_multi_inputs", "blsw_engine_create_multi_inputs",
                    "blsw_compact_layout_multi", "blsw_compact_locate_multi", "blsw_compact_locate_multi_range", "blsw_r1cs_pair_families",
                    "blsw_r1cs_handle_pair_families", "blsw_r1cs_check_compact_multi", "blsw_r1cs_check_compact_multi_ex", "blsw_r1cs_evaluate_compact_multi",
                    "blsw_registry_bytes", "blsw_registry_create", "blsw_registry_append", "blsw_registry_size", "blsw_registry_key_status", "blsw_registry_destroy",
                    "blsw_registry_verify_workspace_bytes", "blsw_registry_verify_batch", "blsw_verify_pairs_workspace_bytes", "blsw_verify_pairs_batch",
                    "blsw_dst_set", "blsw_dst_default", "blsw_dst_pop", "blsw_hash_to_field_batch", "blsw_pop_prove_batch", "blsw_pop_verify_batch",
                    "blsw_verify_groups_shared_workspace_bytes", "blsw_verify_groups_shared_batch", "blsw_registry_verify_shared_workspace_bytes",
                    "blsw_registry_verify_shared_batch", "blsw_combine_points_workspace_bytes", "blsw_combine_points_batch", "blsw_lagrange_batch",
                    "blsw_recover_points_batch", "blsw_msm_workspace_bytes", "blsw_msm_points_batch",
                    "blsw_registry_msm_workspace_bytes", "blsw_registry_msm_batch"] + [e + "_dst" for e in _DST_ENTRIES]

DST_DEFAULT = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"  # the library's tag: what every value entry hashes under with dst=None
DST_POP = b"BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"  # PopProve / PopVerify of the signature draft


def _dst_struct(dst):
    """bytes of 1 .. 255 -> blsw_dst_t (blsw_dst_set states the rule)"""
    t = blsw_dst_t()
    raw = bytes(dst)
    rc = lib().blsw_dst_set(ctypes.byref(t), raw, len(raw))
    if rc:
        raise BlswError("blsw_dst_set failed: %d (a tag has 1 .. 255 bytes, this one %d)" % (rc, len(raw)))
    return t


def _dst_entry(name, dst):
    """the C entry `name` for dst=None — the call is then exactly what it was — or its _dst form with the tag bound in front of the stream"""
    if dst is None:
        return getattr(lib(), name)
    fn, t = getattr(lib(), name + "_dst"), _dst_struct(dst)
    return lambda *a: fn(*a[:-1], ctypes.byref(t), a[-1])


PARAMS_MODES = {"constant": 0, "witness": 1}
IO_MODES = {"witness": 0, "input": 1, "Witness": 0, "Input": 1}


AGG_KEYS_INPUT, AGG_BITMAP_INPUT, AGG_MSG_INPUT, AGG_SIG_INPUT = 1, 2, 4, 8  # include/blsw.h: BLSW_AGG_*_INPUT, the bits of agg_inputs
MULTI_KEYS_INPUT, MULTI_MSG_INPUT, MULTI_SIG_INPUT = 1, 4, 8  # include/blsw.h: BLSW_MULTI_*_INPUT, the bits of multi_inputs


def layout(msg_len=32, params_mode=0, pk_mode=0, sig_mode=0, msg_mode=0):
    """Segment table of the witness vector (host logic; replaces cs.num_witness_variables(), constraints.rs:369-373).
    params_mode 1 / "witness": ParametersVar::new_variable with AllocationMode::Witness (constraints.rs:198-211).
    pk_mode / sig_mode 1 / "input": PublicKeyVar / SignatureVar::new_variable with AllocationMode::Input (constraints.rs:214-249): the point's
    coordinates are public inputs (n_instance_vars > 1), its allocation segment is empty.
    msg_mode 1 / "input": UInt8::new_input_vec (constraints.rs:341 with AllocationMode::Input; blsw_layout_inputs): the message is
    msg_input_chunks(msg_len) public inputs in front of the key's and the signature's, its segment 761 witnesses per chunk."""
    L = blsw_layout_t()
    params_mode = PARAMS_MODES.get(params_mode, params_mode)
    pk_mode, sig_mode, msg_mode = IO_MODES.get(pk_mode, pk_mode), IO_MODES.get(sig_mode, sig_mode), IO_MODES.get(msg_mode, msg_mode)
    if msg_mode:
        if params_mode:
            raise BlswError("msg_mode Input applies to the circuit with Constant parameters")
        rc = lib().blsw_layout_inputs(msg_len, msg_mode, pk_mode, sig_mode, ctypes.byref(L))
    elif pk_mode or sig_mode:
        if params_mode:
            raise BlswError("pk_mode / sig_mode Input apply to the circuit with Constant parameters")
        rc = lib().blsw_layout_io(msg_len, pk_mode, sig_mode, ctypes.byref(L))
    else:
        rc = lib().blsw_layout_params(msg_len, params_mode, ctypes.byref(L)) if params_mode else lib().blsw_layout(msg_len, ctypes.byref(L))
    if rc:
        raise BlswError("blsw_layout failed: %d" % rc)
    return {n: getattr(L, n) for n in _LAYOUT_FIELDS}


MSG_CHUNK_BYTES = 47  # UInt8::new_input_vec: bytes per public input, (MODULUS_BIT_SIZE - 1) / 8


def msg_input_chunks(msg_len):
    """public inputs of a message of msg_len bytes allocated with UInt8::new_input_vec (= n_instance_vars - 1 - 3 pk_mode - 6 sig_mode)"""
    return (int(msg_len) + MSG_CHUNK_BYTES - 1) // MSG_CHUNK_BYTES


def engine_workspace_bytes(n, msg_len=32, max_steps=1, n_buffers=1):
    b = ctypes.c_uint64(0)
    rc = lib().blsw_engine_workspace_bytes(n, msg_len, max_steps, n_buffers, ctypes.byref(b))
    if rc:
        raise BlswError("blsw_engine_workspace_bytes failed: %d" % rc)
    return b.value


def _require_cuda():
    import torch

    if not torch.cuda.is_available():
        raise BlswError("no HIP device visible: the witness path runs only on the GPU (there is no CPU fallback)")
    return torch


def check_capacity(device, what, *byte_counts):
    """Refuses (BlswError) before anything is allocated when the buffers a direct call needs — its workspace and, with want_witness, n witness
    vectors (a 128-pair instance is 4.19 GB) — exceed the free HBM of `device`: a clear error instead of an allocator exception half-way."""
    torch = _require_cuda()
    need = int(sum(byte_counts))
    free_b, _ = torch.cuda.mem_get_info(device)
    # memory torch has cached but not in use is reusable by the allocations that follow
    reusable = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    if need > free_b + reusable:
        raise BlswError("%s needs %.2f GB of HBM (workspace + witness vectors) and %.2f GB are free on %s: pass fewer instances per call, "
                        "want_witness=False, or stream the batch through a WitnessEngine with a small ring of outputs" % (what, need / 1e9, (free_b + reusable) / 1e9, device))


def engine_options(**overrides):
    """blsw_engine_options_default with keyword overrides: device, pairing_mode ("team"/"lane" or 0/1), g2_mode ("lane"/"team"
    or 0/1), expand_variant, expand_store, prio_mode, place_lds, consumer_mode, output_form, n_keys, agg_inputs (mask of AGG_*_INPUT), n_pairs. The library itself reads no
    environment for its options (one diagnostic: BLSW_TRACE_GROUP=1 prints every launch group's stage times at engine destruction); for A/B runs of measurement scripts THIS function applies BLSW_PAIRING=lane, BLSW_G2=team, BLSW_EXPAND_VARIANT,
    BLSW_EXPAND_NT, BLSW_PRIO_MODE, BLSW_PLACE_LDS (explicit keyword arguments win)."""
    o = blsw_engine_options_t()
    rc = lib().blsw_engine_options_default(ctypes.byref(o))
    if rc:
        raise BlswError("blsw_engine_options_default failed: %d" % rc)
    env = os.environ
    if env.get("BLSW_PAIRING", "")[:1] == "l":
        o.pairing_mode = 1
    if env.get("BLSW_G2", "")[:1] == "t" and o.pairing_mode == 0:
        o.g2_mode = 1
    for var, field in (("BLSW_CHAIN_VARIANT", "chain_variant"), ("BLSW_COFACTOR_MODE", "cofactor_mode"), ("BLSW_EXPAND_VARIANT", "expand_variant"), ("BLSW_EXPAND_NT", "expand_store"), ("BLSW_PRIO_MODE", "prio_mode"), ("BLSW_PLACE_LDS", "place_lds"), ("BLSW_GROUP_RAMP", "group_ramp"), ("BLSW_LATENCY_MODE", "latency_mode")):
        if env.get(var):
            setattr(o, field, int(env[var]))
    names = {"pairing_mode": {"team": 0, "lane": 1}, "g2_mode": {"lane": 0, "team": 1}, "params_mode": PARAMS_MODES, "pk_mode": IO_MODES, "sig_mode": IO_MODES,
             "msg_mode": IO_MODES}
    for k, v in overrides.items():
        if v is None:
            continue
        if not hasattr(o, k):
            raise BlswError("unknown engine option %r" % k)
        setattr(o, k, names.get(k, {}).get(v, v))
    return o


def compact_layout(n, msg_len=32, **options):
    """blsw_compact_layout: where every witness element of a compact step of n instances lives (blsw_compact_layout_t), for the engine options given
    as in WitnessEngine(...). Host only."""
    opt = options.pop("_opt", None) or engine_options(**options)
    c = blsw_compact_layout_t()
    rc = lib().blsw_compact_layout(n, msg_len, ctypes.byref(opt), ctypes.byref(c))
    if rc:
        raise BlswError("blsw_compact_layout failed: %d" % rc)
    return c


def compact_layout_keyset(n, msg_len=32, **options):
    """blsw_compact_layout_keyset -> (layout, head_len) of the compact steps of a shared-keys engine (options with shared_keys=1): the layout of the
    buffer, which carries no key rows, and the length of the head the receiver's KeySet supplies. Witness k of the caller's vector is table[k] for
    k < head_len, else compact_locate(layout, k - head_len, lane). Host only."""
    opt = options.pop("_opt", None) or engine_options(**options)
    c, head = blsw_compact_layout_t(), ctypes.c_uint32(0)
    rc = lib().blsw_compact_layout_keyset(n, msg_len, ctypes.byref(opt), ctypes.byref(c), ctypes.byref(head))
    if rc:
        raise BlswError("blsw_compact_layout_keyset failed: %d" % rc)
    return c, head.value


def compact_locate(layout, k, lane):
    """blsw_compact_locate -> (region COMPACT_BIT / _TILE / _PAIR, byte offset in the buffer, bit position in the u32 word at that offset)"""
    region, off, bit = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = lib().blsw_compact_locate(ctypes.byref(layout), k, lane, ctypes.byref(region), ctypes.byref(off), ctypes.byref(bit))
    if rc:
        raise BlswError("blsw_compact_locate failed: %d" % rc)
    return region.value, off.value, bit.value


def compact_locate_all(layout, lane):
    """compact_locate of every witness index for one lane -> (region uint8 [n_witness], byte offset int64 [n_witness], bit uint8 [n_witness])"""
    import numpy as np

    nw = layout.n_witness
    region, off, bit = np.zeros(nw, np.uint8), np.zeros(nw, np.int64), np.zeros(nw, np.uint8)
    r, o, b = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    fn, lp, rp, op, bp = lib().blsw_compact_locate, ctypes.byref(layout), ctypes.byref(r), ctypes.byref(o), ctypes.byref(b)
    for k in range(nw):
        if fn(lp, k, lane, rp, op, bp):
            raise BlswError("blsw_compact_locate failed at k = %d" % k)
        region[k], off[k], bit[k] = r.value, o.value, b.value
    return region, off, bit


def compact_layout_multi(n, msg_len=32, n_pairs=None, multi_inputs=0, **options):
    """blsw_compact_layout_multi: where every witness element of a compact step of n instances of the N+1-pair product lives
    (blsw_compact_layout_multi_t), for the engine arguments given as in WitnessEngine(..., n_pairs=K, multi_inputs=mask). Host only."""
    opt = options.pop("_opt", None) or engine_options(n_pairs=n_pairs, **options)
    c = blsw_compact_layout_multi_t()
    rc = lib().blsw_compact_layout_multi(n, msg_len, ctypes.byref(opt), multi_inputs, ctypes.byref(c))
    if rc:
        raise BlswError("blsw_compact_layout_multi failed: %d" % rc)
    return c


def compact_locate_multi(layout, k, instance):
    """blsw_compact_locate_multi -> (region COMPACT_BIT / _TILE / _INST / _PAIR, byte offset in the buffer, bit position in the u32 word at that offset)"""
    region, off, bit = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = lib().blsw_compact_locate_multi(ctypes.byref(layout), k, instance, ctypes.byref(region), ctypes.byref(off), ctypes.byref(bit))
    if rc:
        raise BlswError("blsw_compact_locate_multi failed: %d" % rc)
    return region.value, off.value, bit.value


def compact_locate_multi_all(layout, instance, k_begin=0, count=None):
    """compact_locate_multi of witnesses [k_begin, k_begin + count) (default: all) of one instance -> (region uint8, byte offset uint64, bit uint8)"""
    import numpy as np

    count = layout.n_witness - k_begin if count is None else count
    region, off, bit = np.empty(count, np.uint8), np.empty(count, np.uint64), np.empty(count, np.uint8)
    rc = lib().blsw_compact_locate_multi_range(ctypes.byref(layout), k_begin, count, instance, region.ctypes.data, off.ctypes.data, bit.ctypes.data)
    if rc:
        raise BlswError("blsw_compact_locate_multi_range failed: %d" % rc)
    return region, off, bit


SEG_PK_ALLOC = 1942  # witnesses of one G1Var::new_variable(Witness): a key's block of the keys segment and of a KeySet's table


def keyset_bytes(n_keys):
    b = ctypes.c_uint64(0)
    rc = lib().blsw_keyset_bytes(n_keys, ctypes.byref(b))
    if rc:
        raise BlswError("blsw_keyset_bytes failed: %d" % rc)
    return b.value


class KeySet:
    """A key set shared by many aggregate_verify instances (blsw_keyset_*): pks_xy [K, 12] int64 affine Montgomery, (0, 0) = the point at infinity.
    Its keys' allocation witnesses are computed once, on the current stream of `device`; a WitnessEngine(..., n_keys=K, shared_keys=1) of the same
    output_form copies them into every instance's vector (submit_aggregate_keyset). .table: [K * 1942, 6] int64 view of the table."""

    def __init__(self, pks_xy, device=None, output_form=0):
        torch = _require_cuda()
        assert pks_xy.dim() == 2 and pks_xy.shape[1] == 12 and pks_xy.shape[0] >= 1
        self.device = torch.device(device if device is not None else (pks_xy.device if pks_xy.is_cuda else "cuda:%d" % torch.cuda.current_device()))
        self.pks_xy = pks_xy.to(self.device).contiguous()
        self.n_keys, self.output_form = int(pks_xy.shape[0]), int(output_form)
        self.buffer = torch.empty(keyset_bytes(self.n_keys), dtype=torch.uint8, device=self.device)  # the allocator's blocks are 512-byte aligned
        self._ks = ctypes.c_void_p()
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        rc = lib().blsw_keyset_create(ctypes.byref(self._ks), self.pks_xy.data_ptr(), self.n_keys, self.output_form, index, self.buffer.data_ptr(), self.buffer.numel(),
                                      torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            self._ks = None
            raise BlswError("blsw_keyset_create failed: %d" % rc)
        ptr, n_el = ctypes.c_void_p(), ctypes.c_uint64(0)
        rc = lib().blsw_keyset_table(self._ks, ctypes.byref(ptr), ctypes.byref(n_el))
        if rc or ptr.value != self.buffer.data_ptr() or n_el.value != self.n_keys * SEG_PK_ALLOC:
            raise BlswError("blsw_keyset_table failed: %d" % rc)
        self.table = self.buffer[:n_el.value * FP_BYTES].view(torch.int64).view(n_el.value, 6)

    def broadcast_rate(self, witness, order=0, reps=3):
        """blsw_keyset_broadcast_rate: bytes per second the table is written into the heads of `witness` [n, stride, 6] at (order 0: what the engine launches)"""
        r = ctypes.c_double(0)
        rc = lib().blsw_keyset_broadcast_rate(self._ks, witness.data_ptr(), witness.shape[1], witness.shape[0], order, reps, ctypes.byref(r))
        if rc:
            raise BlswError("blsw_keyset_broadcast_rate failed: %d" % rc)
        return r.value

    def close(self):
        if getattr(self, "_ks", None):
            lib().blsw_keyset_destroy(self._ks)
            self._ks = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WitnessEngine:
    """Thin wrapper of blsw_engine_*: submit batches, flush, read results. max_steps batches are fused per launch group.
    Streaming consumers use the step numbers returned by submit(): wait_step(seq) / output_consumed(tensor)."""

    def __init__(self, n, msg_len=32, max_steps=1, device=None, n_buffers=None, reserve_bytes=0, **options):
        """options: fields of blsw_engine_options_t; n_keys=K makes it an aggregate_verify engine (submit_aggregate). multi_inputs=mask (with n_pairs=K,
        MULTI_*_INPUT): the N+1-pair product with Input arguments — no field of the struct, the argument of blsw_engine_create_multi_inputs.
        reserve_bytes: bytes the caller will allocate next to the workspace (its witness tensors): the capacity check, made with the byte count
        blsw_engine_workspace_bytes_ex returns for THESE options and this n_buffers, covers them too (BlswError instead of an allocator exception)."""
        torch = _require_cuda()
        self.torch = torch
        self.n, self.msg_len, self.max_steps = int(n), int(msg_len), int(max_steps)
        self.n_buffers = int(n_buffers) if n_buffers is not None else (3 if self.max_steps > 1 else 1)
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.multi_inputs = int(options.pop("multi_inputs", 0) or 0)
        opt = engine_options(**options)
        opt.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._opt = opt
        self.n_keys = int(opt.n_keys)
        self.n_pairs = int(opt.n_pairs) if opt.n_pairs > 1 else 1
        self.msg_mode = int(opt.msg_mode)
        self.agg_inputs = int(opt.agg_inputs)
        self.shared_keys = int(opt.shared_keys)
        self.layout = layout_aggregate(msg_len, self.n_keys, self.agg_inputs) if self.n_keys else (layout_multi(msg_len, self.n_pairs, self.multi_inputs) if self.n_pairs > 1 else
                                                                                  layout(msg_len, int(opt.params_mode), int(opt.pk_mode), int(opt.sig_mode), self.msg_mode))
        self.n_witness = self.layout["n_witness"]
        self.n_instance_vars = self.layout["n_instance_vars"]
        wb = ctypes.c_uint64(0)
        rc = lib().blsw_engine_workspace_bytes_multi_inputs(self.n, self.msg_len, self.max_steps, self.n_buffers, ctypes.byref(opt), self.multi_inputs, ctypes.byref(wb))
        if rc:
            raise BlswError("blsw_engine_workspace_bytes_ex failed: %d" % rc)
        check_capacity(self.device, "WitnessEngine (n = %d, max_steps = %d, n_buffers = %d)" % (self.n, self.max_steps, self.n_buffers), wb.value, reserve_bytes)
        self.workspace = torch.empty(wb.value, dtype=torch.uint8, device=self.device)
        self._e = ctypes.c_void_p()
        rc = lib().blsw_engine_create_multi_inputs(ctypes.byref(self._e), self.n, self.msg_len, self.max_steps, self.n_buffers, ctypes.byref(opt), self.multi_inputs,
                                                   self.workspace.data_ptr(), self.workspace.numel())
        if rc:
            self._e = None
            raise BlswError("blsw_engine_create_ex failed: %d" % rc)
        self._keep = []

    def close(self):
        if getattr(self, "_e", None):
            lib().blsw_engine_destroy(self._e)
            self._e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def new_witness_tensor(self):
        return self.torch.empty((self.n, self.n_witness, 6), dtype=self.torch.int64, device=self.device)

    def new_instance_tensor(self):
        """[n, n_instance_vars, 6]: instance_assignment of every instance (submit(..., instance=...); element 0 = one)"""
        return self.torch.empty((self.n, self.n_instance_vars, 6), dtype=self.torch.int64, device=self.device)

    def _stream(self, stream):
        return (stream if stream is not None else self.torch.cuda.current_stream(self.device)).cuda_stream

    def submit(self, pk_xy, sig_xy, msg, witness=None, result=None, stream=None, instance=None):
        """-> step number (0, 1, 2, ... in submission order). instance: [n, n_instance_vars, 6] tensor that receives instance_assignment
        (blsw_engine_submit_io; msg_mode / pk_mode / sig_mode Input engines: the public inputs an arkworks verifier takes)."""
        assert pk_xy.is_cuda and sig_xy.is_cuda and msg.is_cuda
        assert pk_xy.shape == (self.n, 12) and sig_xy.shape == (self.n, 24) and msg.shape == (self.n, self.msg_len)
        assert pk_xy.is_contiguous() and sig_xy.is_contiguous() and msg.is_contiguous()
        if witness is not None:
            assert witness.is_contiguous() and witness.shape[0] == self.n and witness.shape[1] >= self.n_witness
        if result is not None:
            assert result.is_contiguous() and result.numel() >= self.n
        seq = self.submitted()
        if instance is not None:
            assert instance.is_contiguous() and tuple(instance.shape) == (self.n, self.n_instance_vars, 6)
            rc = lib().blsw_engine_submit_io(self._e, pk_xy.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None, instance.data_ptr(),
                                             witness.data_ptr() if witness is not None else None, witness.shape[1] if witness is not None else 0,
                                             result.data_ptr() if result is not None else None, self._stream(stream))
        else:
            rc = lib().blsw_engine_submit(self._e, pk_xy.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None,
                                          witness.data_ptr() if witness is not None else None, witness.shape[1] if witness is not None else 0,
                                          result.data_ptr() if result is not None else None, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit failed: %d" % rc)
        self._keep.append((pk_xy, sig_xy, msg, witness, result))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def submit_bytes(self, pk48, sig96, msg, witness=None, result=None, stream=None):
        """blsw_engine_submit_bytes: compressed points [n, 48] / [n, 96] uint8 -> (step number, pk_xy, sig_xy, status [n, 2]);
        result[i] = 1 iff both points decode to non-identity subgroup points and the gadget's Boolean is true (tests.rs:244-263)."""
        torch = self.torch
        assert pk48.shape == (self.n, 48) and sig96.shape == (self.n, 96) and msg.shape == (self.n, self.msg_len)
        assert pk48.is_contiguous() and sig96.is_contiguous() and msg.is_contiguous() and pk48.dtype == torch.uint8 and sig96.dtype == torch.uint8
        if witness is not None:
            assert witness.is_contiguous() and witness.shape[0] == self.n and witness.shape[1] >= self.n_witness
        pk_xy = torch.empty((self.n, 12), dtype=torch.int64, device=self.device)
        sig_xy = torch.empty((self.n, 24), dtype=torch.int64, device=self.device)
        status = torch.empty((self.n, 2), dtype=torch.int32, device=self.device)
        seq = self.submitted()
        rc = lib().blsw_engine_submit_bytes(self._e, pk48.data_ptr(), sig96.data_ptr(), msg.data_ptr() if self.msg_len else None, pk_xy.data_ptr(), sig_xy.data_ptr(),
                                            status.data_ptr(), witness.data_ptr() if witness is not None else None, witness.shape[1] if witness is not None else 0,
                                            result.data_ptr() if result is not None else None, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_bytes failed: %d" % rc)
        self._keep.append((pk48, sig96, msg, pk_xy, sig_xy, status, witness, result))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq, pk_xy, sig_xy, status

    def submit_multi(self, pks_xy, msgs, sig_xy, witness=None, result=None, stream=None, instance=None):
        """N+1-pair product batch (engine created with n_pairs=K): pks_xy [n, K, 12] int64, msgs [n, K, msg_len] uint8, sig_xy [n, 24] -> step number.
        instance: [n, n_instance_vars, 6] tensor that receives instance_assignment (blsw_engine_submit_multi_io; multi_inputs engines: the message
        chunks, keys and signature an arkworks verifier takes as public inputs, in that order)."""
        K = self.n_pairs
        assert K > 1 and pks_xy.shape == (self.n, K, 12) and msgs.shape == (self.n, K, self.msg_len) and sig_xy.shape == (self.n, 24)
        assert pks_xy.is_contiguous() and msgs.is_contiguous() and sig_xy.is_contiguous()
        if witness is not None:
            assert witness.is_contiguous() and witness.shape[0] == self.n and witness.shape[1] >= self.n_witness
        seq = self.submitted()
        tail = (witness.data_ptr() if witness is not None else None, witness.shape[1] if witness is not None else 0,
                result.data_ptr() if result is not None else None, self._stream(stream))
        if instance is not None:
            assert instance.is_contiguous() and tuple(instance.shape) == (self.n, self.n_instance_vars, 6)
            rc = lib().blsw_engine_submit_multi_io(self._e, pks_xy.data_ptr(), msgs.data_ptr() if self.msg_len else None, sig_xy.data_ptr(), instance.data_ptr(), *tail)
        else:
            rc = lib().blsw_engine_submit_multi(self._e, pks_xy.data_ptr(), msgs.data_ptr() if self.msg_len else None, sig_xy.data_ptr(), *tail)
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_multi failed: %d" % rc)
        self._keep.append((pks_xy, msgs, sig_xy, witness, result, instance))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def submit_multi_compact(self, pks_xy, msgs, sig_xy, compact, result=None, stream=None):
        """submit_multi with the step's compact wire form in `compact` (uint8 tensor of compact_bytes()) as its output -> step number"""
        K = self.n_pairs
        assert K > 1 and pks_xy.shape == (self.n, K, 12) and msgs.shape == (self.n, K, self.msg_len) and sig_xy.shape == (self.n, 24)
        assert pks_xy.is_contiguous() and msgs.is_contiguous() and sig_xy.is_contiguous()
        assert compact.is_cuda and compact.is_contiguous() and compact.dtype.itemsize == 1 and compact.numel() >= self.compact_bytes()
        seq = self.submitted()
        rc = lib().blsw_engine_submit_multi_compact(self._e, pks_xy.data_ptr(), msgs.data_ptr() if self.msg_len else None, sig_xy.data_ptr(), compact.data_ptr(),
                                                    result.data_ptr() if result is not None else None, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_multi_compact failed: %d" % rc)
        self._keep.append((pks_xy, msgs, sig_xy, compact, result))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def submit_aggregate(self, pks_xy, bitmap, sig_xy, msg, witness=None, result=None, count=None, stream=None, instance=None):
        """aggregate_verify batch (engine created with n_keys=K): pks_xy [n, K, 12] int64, bitmap [n, K] uint8 -> step number.
        instance: [n, n_instance_vars, 6] tensor that receives instance_assignment (blsw_engine_submit_aggregate_io; agg_inputs engines: the
        keys, bitmap bits, message chunks and signature an arkworks verifier takes as public inputs, in that order)."""
        K = self.n_keys
        assert K and pks_xy.shape == (self.n, K, 12) and bitmap.shape == (self.n, K) and sig_xy.shape == (self.n, 24) and msg.shape == (self.n, self.msg_len)
        assert pks_xy.is_contiguous() and bitmap.is_contiguous() and sig_xy.is_contiguous() and msg.is_contiguous()
        if witness is not None:
            assert witness.is_contiguous() and witness.shape[0] == self.n and witness.shape[1] >= self.n_witness
        seq = self.submitted()
        tail = (witness.data_ptr() if witness is not None else None, witness.shape[1] if witness is not None else 0,
                result.data_ptr() if result is not None else None, count.data_ptr() if count is not None else None, self._stream(stream))
        if instance is not None:
            assert instance.is_contiguous() and tuple(instance.shape) == (self.n, self.n_instance_vars, 6)
            rc = lib().blsw_engine_submit_aggregate_io(self._e, pks_xy.data_ptr(), bitmap.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None,
                                                       instance.data_ptr(), *tail)
        else:
            rc = lib().blsw_engine_submit_aggregate(self._e, pks_xy.data_ptr(), bitmap.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None, *tail)
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_aggregate failed: %d" % rc)
        self._keep.append((pks_xy, bitmap, sig_xy, msg, witness, result, count, instance))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def _keyset_step(self, keyset, bitmap, sig_xy, msg):
        K = self.n_keys
        assert isinstance(keyset, KeySet) and K and bitmap.shape == (self.n, K) and sig_xy.shape == (self.n, 24) and msg.shape == (self.n, self.msg_len)
        assert bitmap.is_contiguous() and sig_xy.is_contiguous() and msg.is_contiguous()

    def submit_aggregate_keyset(self, keyset, bitmap, sig_xy, msg, witness=None, result=None, count=None, stream=None, instance=None):
        """submit_aggregate of an engine created with shared_keys=1: the step's keys are `keyset` (a KeySet of this engine's n_keys, output_form and
        device; the steps of one launch group may name different sets) -> step number. The vectors are those of submit_aggregate with the keys
        replicated [n, K, 12]. The set's table must be complete on, or ordered before, the submitting stream."""
        self._keyset_step(keyset, bitmap, sig_xy, msg)
        if witness is not None:
            assert witness.is_contiguous() and witness.shape[0] == self.n and witness.shape[1] >= self.n_witness
        if instance is not None:
            assert instance.is_contiguous() and tuple(instance.shape) == (self.n, self.n_instance_vars, 6)
        seq = self.submitted()
        rc = lib().blsw_engine_submit_aggregate_keyset(self._e, keyset._ks, bitmap.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None,
                                                       instance.data_ptr() if instance is not None else None, witness.data_ptr() if witness is not None else None,
                                                       witness.shape[1] if witness is not None else 0, result.data_ptr() if result is not None else None,
                                                       count.data_ptr() if count is not None else None, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_aggregate_keyset failed: %d" % rc)
        self._keep.append((keyset, bitmap, sig_xy, msg, witness, result, count, instance))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def submit_aggregate_keyset_compact(self, keyset, bitmap, sig_xy, msg, compact, result=None, count=None, stream=None):
        """submit_aggregate_keyset with the step's compact wire form in `compact` as its output (no key rows: the receiver's expand_compact takes
        the set) -> step number"""
        self._keyset_step(keyset, bitmap, sig_xy, msg)
        assert compact.is_cuda and compact.is_contiguous() and compact.dtype.itemsize == 1 and compact.numel() >= self.compact_bytes()
        seq = self.submitted()
        rc = lib().blsw_engine_submit_aggregate_keyset_compact(self._e, keyset._ks, bitmap.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None,
                                                               compact.data_ptr(), result.data_ptr() if result is not None else None,
                                                               count.data_ptr() if count is not None else None, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_aggregate_keyset_compact failed: %d" % rc)
        self._keep.append((keyset, bitmap, sig_xy, msg, compact, result, count))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def compact_bytes(self):
        """Bytes of one batch in compact wire form (bit-packed SHA witnesses + staged field witnesses, ~2.6 MB per instance)."""
        return self._counter(lib().blsw_engine_compact_bytes)

    def compact_layout(self):
        """blsw_compact_layout_t of this engine's compact steps (ConstraintChecker.which_is_unsatisfied_compact reads a step through it). A shared-keys
        engine: the layout of the buffer alone (compact_layout_keyset; the head is the step's KeySet, passed to the checker as keyset=)."""
        if self._opt.shared_keys:
            return compact_layout_keyset(self.n, self.msg_len, _opt=self._opt)[0]
        if self.n_pairs > 1:  # the N+1-pair product: blsw_compact_layout_multi_t, which the same checker calls take
            return compact_layout_multi(self.n, self.msg_len, multi_inputs=self.multi_inputs, _opt=self._opt)
        return compact_layout(self.n, self.msg_len, _opt=self._opt)

    def new_compact_buffer(self, batches=1):
        import torch

        return torch.empty((batches, self.compact_bytes()), dtype=torch.uint8, device=self.device)

    def submit_compact(self, pk_xy, sig_xy, msg, compact, result=None, stream=None):
        """As submit(), but the step's output is its compact wire form in `compact` (uint8 tensor of compact_bytes()) -> step number"""
        assert pk_xy.shape == (self.n, 12) and sig_xy.shape == (self.n, 24) and msg.shape == (self.n, self.msg_len)
        assert pk_xy.is_contiguous() and sig_xy.is_contiguous() and msg.is_contiguous()
        assert compact.is_cuda and compact.is_contiguous() and compact.dtype.itemsize == 1 and compact.numel() >= self.compact_bytes()
        seq = self.submitted()
        rc = lib().blsw_engine_submit_compact(self._e, pk_xy.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None, compact.data_ptr(),
                                              result.data_ptr() if result is not None else None, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_compact failed: %d" % rc)
        self._keep.append((pk_xy, sig_xy, msg, compact, result))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def submit_aggregate_compact(self, pks_xy, bitmap, sig_xy, msg, compact, result=None, count=None, stream=None):
        """submit_aggregate with the step's compact wire form in `compact` as its output -> step number"""
        K = self.n_keys
        assert K and pks_xy.shape == (self.n, K, 12) and bitmap.shape == (self.n, K) and sig_xy.shape == (self.n, 24) and msg.shape == (self.n, self.msg_len)
        assert pks_xy.is_contiguous() and bitmap.is_contiguous() and sig_xy.is_contiguous() and msg.is_contiguous()
        assert compact.is_cuda and compact.is_contiguous() and compact.dtype.itemsize == 1 and compact.numel() >= self.compact_bytes()
        seq = self.submitted()
        rc = lib().blsw_engine_submit_aggregate_compact(self._e, pks_xy.data_ptr(), bitmap.data_ptr(), sig_xy.data_ptr(), msg.data_ptr() if self.msg_len else None,
                                                        compact.data_ptr(), result.data_ptr() if result is not None else None,
                                                        count.data_ptr() if count is not None else None, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_submit_aggregate_compact failed: %d" % rc)
        self._keep.append((pks_xy, bitmap, sig_xy, msg, compact, result, count))
        self._keep = self._keep[-(self.n_buffers + 1) * self.max_steps:]
        return seq

    def expand_compact(self, compact, witness, stream=None, keyset=None):
        """Receiver side: one batch in compact form (this engine's or another rank's) -> its n witness vectors in `witness`.
        keyset: the step's KeySet (engines with shared_keys=1: the compact form carries no key rows)."""
        assert compact.is_cuda and compact.is_contiguous() and compact.numel() >= self.compact_bytes()
        assert witness.is_contiguous() and witness.shape[0] == self.n and witness.shape[1] >= self.n_witness
        if keyset is not None:
            rc = lib().blsw_engine_expand_compact_keyset(self._e, keyset._ks, compact.data_ptr(), witness.data_ptr(), witness.shape[1], self._stream(stream))
        else:
            rc = lib().blsw_engine_expand_compact(self._e, compact.data_ptr(), witness.data_ptr(), witness.shape[1], self._stream(stream))
        if rc:
            raise BlswError("blsw_engine_expand_compact failed: %d" % rc)

    def flush(self, stream=None):
        rc = lib().blsw_engine_flush(self._e, self._stream(stream))
        if rc:
            raise BlswError("blsw_engine_flush failed: %d" % rc)

    def _counter(self, fn):
        v = ctypes.c_uint64(0)
        rc = fn(self._e, ctypes.byref(v))
        if rc:
            raise BlswError("engine counter failed: %d" % rc)
        return v.value

    def submitted(self):
        return self._counter(lib().blsw_engine_submitted)

    def launched(self):
        return self._counter(lib().blsw_engine_launched)

    def materialised(self):
        """Steps whose output writes have been issued (= launched() unless consumer_mode holds steps back for their outputs)."""
        return self._counter(lib().blsw_engine_materialised)

    def wait_step(self, seq, stream=None):
        """Makes `stream` (default: the current stream) wait for step `seq`'s witness tensor and results (seq < launched())."""
        rc = lib().blsw_engine_wait_step(self._e, seq, self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_wait_step failed: %d" % rc)

    def output_consumed(self, witness, stream=None):
        """The consumer is done with `witness` once `stream` reaches this point: the next step submitted with the same tensor
        does not overwrite it earlier."""
        rc = lib().blsw_engine_output_consumed(self._e, witness.data_ptr(), self._stream(stream))
        if rc:
            raise (BlswBusy if rc == ERR_BUSY else BlswError)("blsw_engine_output_consumed failed: %d" % rc)

    def expand_stats(self):
        """(number of k_sha_expand launches since the last call, their average duration in ms); synchronises with them."""
        ms, cnt = ctypes.c_float(0), ctypes.c_uint32(0)
        rc = lib().blsw_engine_expand_stats(self._e, ctypes.byref(cnt), ctypes.byref(ms))
        if rc:
            raise BlswError("blsw_engine_expand_stats failed: %d" % rc)
        return cnt.value, ms.value


class ParametersVar:
    """constraints.rs:23-28, AllocVar at :194-212: the default generator, allocated as a Constant (every circuit of the reference) or
    as a Witness (new_witness: the generator goes through G1Var::new_variable like a public key). AllocationMode::Input would put it
    into instance_assignment, which the engine does not produce."""

    def __init__(self, mode="Constant"):
        if mode not in ("Constant", "Witness"):
            raise BlswError("ParametersVar: AllocationMode %r is not on the GPU path (Constant or Witness)" % (mode,))
        self.mode = mode

    @classmethod
    def new_constant(cls):
        return cls("Constant")

    @classmethod
    def new_witness(cls):
        return cls("Witness")


class PublicKeyVar:
    """constraints.rs:39-44, AllocVar at :214-232: Witness (the reference's circuits) or Input (new_input: the key's x, y, z are public inputs,
    no in-circuit subgroup check). `xy`: [n, 12] int64 tensor (u64 limbs: x, y Montgomery). AllocationMode::Constant is not on the GPU path."""

    def __init__(self, xy, mode="Witness"):
        if mode not in ("Witness", "Input"):
            raise BlswError("PublicKeyVar: AllocationMode %r is not on the GPU path (Witness or Input)" % (mode,))
        self.xy = xy
        self.mode = mode

    @classmethod
    def new_witness(cls, xy):
        return cls(xy)

    @classmethod
    def new_input(cls, xy):
        return cls(xy, "Input")


class SignatureVar:
    """constraints.rs:55-60, AllocVar at :234-249: Witness or Input (new_input). `xy`: [n, 24] int64 tensor (x.c0, x.c1, y.c0, y.c1)."""

    def __init__(self, xy, mode="Witness"):
        if mode not in ("Witness", "Input"):
            raise BlswError("SignatureVar: AllocationMode %r is not on the GPU path (Witness or Input)" % (mode,))
        self.xy = xy
        self.mode = mode

    @classmethod
    def new_witness(cls, xy):
        return cls(xy)

    @classmethod
    def new_input(cls, xy):
        return cls(xy, "Input")


class UInt8:
    """The message of constraints.rs:341 with its AllocationMode: `bytes` is an [n, msg_len] uint8 tensor. new_witness_vec (the reference's circuits;
    a bare tensor passed to BlsSignatureVerifyGadget.verify means this) or new_input_vec (ark-r1cs-std 0.4.0: each 47-byte chunk is one public
    input, its to_bits_le the witnesses the bytes are made of; the gadget's circuit must be msg_mode="input")."""

    def __init__(self, bytes, mode="Witness"):
        if mode not in ("Witness", "Input"):
            raise BlswError("UInt8: AllocationMode %r is not on the GPU path (Witness or Input)" % (mode,))
        self.bytes = bytes
        self.mode = mode

    @classmethod
    def new_witness_vec(cls, msg):
        return cls(msg)

    @classmethod
    def new_input_vec(cls, msg):
        return cls(msg, "Input")


class Boolean:
    """A bit of aggregate_verify's bitmap (constraints.rs:414-419) with its AllocationMode: `bits` is an [n, K] uint8 tensor of 0 / 1. new_witness (the
    reference's test; a bare tensor passed to aggregate_verify means this) or new_input (AllocatedBool::new_variable with Input: every bit is a public
    input that keeps its booleanity constraint and has no witness)."""

    def __init__(self, bits, mode="Witness"):
        if mode not in ("Witness", "Input"):
            raise BlswError("Boolean: AllocationMode %r is not on the GPU path (Witness or Input)" % (mode,))
        self.bits = bits
        self.mode = mode

    @classmethod
    def new_witness(cls, bits):
        return cls(bits)

    @classmethod
    def new_input(cls, bits):
        return cls(bits, "Input")


class BlsSignatureVerifyGadget:
    """Batched counterpart of constraints.rs:79-128. One call = n independent circuits (direct mode engine, one batch)."""

    def __init__(self, n, msg_len=32, device=None, want_witness=True, max_steps=1, **options):
        """options: blsw_engine_options_t fields; params_mode="witness" builds the circuit for ParametersVar.new_witness(), pk_mode / sig_mode / msg_mode="input"
        the one for PublicKeyVar.new_input / SignatureVar.new_input / UInt8.new_input_vec (self.instance then holds every instance's instance_assignment
        after verify)."""
        reserve = 0
        if want_witness and not options.get("n_keys") and not options.get("n_pairs"):
            reserve = n * layout(msg_len, PARAMS_MODES.get(options.get("params_mode"), options.get("params_mode") or 0), options.get("pk_mode") or 0, options.get("sig_mode") or 0,
                                 options.get("msg_mode") or 0)["n_witness"] * 48
        self.engine = WitnessEngine(n, msg_len, max_steps=max_steps, device=device, reserve_bytes=reserve, **options)
        torch = self.engine.torch
        self.torch = torch
        self.n, self.msg_len, self.device = self.engine.n, self.engine.msg_len, self.engine.device
        self.layout = self.engine.layout
        self.n_witness = self.engine.n_witness
        self.result = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.witness = self.engine.new_witness_tensor() if want_witness else None
        self.instance = self.engine.new_instance_tensor() if self.layout["n_instance_vars"] > 1 else None

    def verify(self, parameters, public_key, message, signature, witness=None, stream=None):
        """message: [n, msg_len] uint8 tensor (UInt8::new_witness_vec) or a UInt8 vector. Returns the int32 result tensor (gadget Boolean per instance);
        the witness vectors are in self.witness (or the tensor passed as `witness`)."""
        assert isinstance(parameters, ParametersVar)
        if (parameters.mode == "Witness") != bool(self.layout["params_mode"]):
            raise BlswError("ParametersVar mode %s does not match the circuit this gadget was built for (params_mode=%d)" % (parameters.mode, self.layout["params_mode"]))
        for var, field in ((public_key, "pk_mode"), (signature, "sig_mode")):
            if (getattr(var, "mode", "Witness") == "Input") != bool(self.layout[field]):
                raise BlswError("%s allocated as %s does not match the circuit this gadget was built for (%s=%d)" % (type(var).__name__, var.mode, field, self.layout[field]))
        msg_var = message if isinstance(message, UInt8) else UInt8(message)
        if (msg_var.mode == "Input") != bool(self.engine.msg_mode):
            raise BlswError("UInt8 vector allocated as %s does not match the circuit this gadget was built for (msg_mode=%d)" % (msg_var.mode, self.engine.msg_mode))
        message = msg_var.bytes
        w = witness if witness is not None else self.witness
        self.engine.submit(public_key.xy, signature.xy, message, witness=w, result=self.result, stream=stream, instance=self.instance)
        self.engine.flush(stream=stream)
        return self.result


def verify_mixed_lengths(parameters, public_key, messages, signature, want_witness=True, **options):
    """`verify` for a batch whose messages differ in LENGTH (constraints.rs:90-95 takes any `&[UInt8]` per call; the circuit — its SHA-256
    block count, hence n_witness and the matrices — is a function of the length, so a batch shares a layout only per length): the
    instances are grouped by message length and each group goes through its own gadget (one engine per distinct length).
    public_key.xy [n, 12], signature.xy [n, 24] cuda tensors; messages: a sequence of n bytes-like objects or 1-D uint8 tensors.
    Returns (result int32 [n], witnesses): witnesses[i] is instance i's [n_witness(len_i), 6] int64 vector (a view of its group's tensor),
    or None with want_witness=False. layout(len(messages[i])) / matrices(len(messages[i])) describe instance i's system."""
    torch = _require_cuda()
    assert isinstance(parameters, ParametersVar)
    if IO_MODES.get(options.get("msg_mode"), options.get("msg_mode")):
        raise BlswError("verify_mixed_lengths: msg_mode Input is not offered (a batch's instance vectors would differ in length)")
    pk, sig = public_key.xy, signature.xy
    n = pk.shape[0]
    if len(messages) != n or sig.shape[0] != n:
        raise BlswError("verify_mixed_lengths: one message and one signature per key")
    dev = pk.device
    groups = {}
    for i, m in enumerate(messages):
        b = bytes(m.cpu().numpy().tobytes()) if hasattr(m, "cpu") else bytes(m)
        groups.setdefault(len(b), []).append((i, b))
    result = torch.empty(n, dtype=torch.int32, device=dev)
    witnesses = [None] * n
    for msg_len, items in sorted(groups.items()):
        idx = torch.tensor([i for i, _ in items], dtype=torch.long, device=dev)
        msg = torch.frombuffer(bytearray(b"".join(b for _, b in items)), dtype=torch.uint8).reshape(len(items), msg_len).to(dev) if msg_len else \
            torch.empty((len(items), 0), dtype=torch.uint8, device=dev)
        g = BlsSignatureVerifyGadget(len(items), msg_len, device=dev, want_witness=want_witness, **options)
        res = g.verify(parameters, PublicKeyVar.new_witness(pk[idx].contiguous()), msg, SignatureVar.new_witness(sig[idx].contiguous()))
        torch.cuda.synchronize(dev)
        result[idx] = res
        if want_witness:
            for k, (i, _) in enumerate(items):
                witnesses[i] = g.witness[k]
        g.engine.close()
    return result, (witnesses if want_witness else None)


ST_OK, ST_BAD_ENCODING, ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP, ST_IDENTITY = 0, 1, 2, 3, 4


def decode_batch(pk48, sig96):
    """PublicKey::try_from / Signature::try_from for a batch (bls.rs:219-242, 316-339): uint8 cuda tensors [n,48], [n,96] ->
    (pk_xy [n,12] int64, sig_xy [n,24] int64, status [n,2] int32)."""
    torch = _require_cuda()
    n = pk48.shape[0]
    assert pk48.shape == (n, 48) and sig96.shape == (n, 96) and pk48.is_contiguous() and sig96.is_contiguous()
    pk_xy = torch.empty((n, 12), dtype=torch.int64, device=pk48.device)
    sig_xy = torch.empty((n, 24), dtype=torch.int64, device=pk48.device)
    status = torch.empty((n, 2), dtype=torch.int32, device=pk48.device)
    rc = lib().blsw_decode_batch(pk48.data_ptr(), sig96.data_ptr(), n, pk_xy.data_ptr(), sig_xy.data_ptr(), status.data_ptr(),
                                 torch.cuda.current_stream(pk48.device).cuda_stream)
    if rc:
        raise BlswError("blsw_decode_batch failed: %d" % rc)
    return pk_xy, sig_xy, status


def aggregate_points(group, points):
    """Signature::aggregate (group 2: [n, k, 96] uint8) / PublicKey::aggregate (group 1: [n, k, 48]) for n lists of k compressed points
    (bls.rs:288-300, 183-195; tests/tests.rs:270-294): returns (sum [n, 96 or 48] uint8, status [n] int32 — ST_OK or the status of the first
    point of the list that does not decode). An empty list (k == 0) is None, as in the reference."""
    torch = _require_cuda()
    nbytes = {1: 48, 2: 96}[group]
    n, k = points.shape[0], points.shape[1]
    assert points.shape == (n, k, nbytes) and points.dtype == torch.uint8 and points.is_contiguous()
    if k == 0:
        return None
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_aggregate_points_workspace_bytes(group, n, k, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_aggregate_points_workspace_bytes failed: %d" % rc)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=points.device)
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=points.device)
    status = torch.empty(n, dtype=torch.int32, device=points.device)
    rc = lib().blsw_aggregate_points_batch(group, points.data_ptr(), k, n, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream(points.device).cuda_stream)
    if rc:
        raise BlswError("blsw_aggregate_points_batch failed: %d" % rc)
    torch.cuda.synchronize(points.device)
    return out, status


def aggregate_signatures(sig96):
    return aggregate_points(2, sig96)


def aggregate_public_keys(pk48):
    return aggregate_points(1, pk48)


ST_BAD_ID = 7  # include/blsw.h: BLSW_ST_BAD_ID, an id that is zero or equal to another id of its list


def _combine_shapes(torch, group, points, rows, counts):
    """the checks combine_points and recover_points share -> (n, k, bytes per point, device)"""
    nbytes = {1: 48, 2: 96}[group]
    n, k = points.shape[0], points.shape[1]
    assert points.shape == (n, k, nbytes) and rows.shape == (n, k, 32) and n > 0 and k > 0
    assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (points, rows)) and rows.device == points.device
    if counts is not None:
        assert counts.shape == (n,) and counts.element_size() == 4 and not counts.is_floating_point() and counts.is_contiguous() and counts.device == points.device
    return n, k, nbytes, points.device


def _combine_workspace(torch, what, group, n, k, dev):
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_combine_points_workspace_bytes(group, n, k, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_combine_points_workspace_bytes failed: %d" % rc)
    check_capacity(dev, "%s (n = %d, %d terms each)" % (what, n, k), wb.value)
    return torch.empty(wb.value, dtype=torch.uint8, device=dev)


def combine_points(group, points, scalars, counts=None, want_term_status=False):
    """sum_j s_j * P_j for n lists of k terms (blsw_combine_points_batch, include/blsw.h): group 1 = public keys ([n, k, 48] uint8), group 2 =
    signatures ([n, k, 96]); scalars [n, k, 32] uint8, little-endian, below r, PUBLIC (the ladders are not constant-time); counts None or an int32 /
    uint32 cuda tensor [n]: list i uses its first counts[i] terms. -> (sum [n, 48 | 96] uint8 — zeros for a failing list, the infinity encoding for a
    sum that is the identity —, status [n] int32[, term_status [n, k, 2] int32: every term's point and scalar decode status])."""
    torch = _require_cuda()
    n, k, nbytes, dev = _combine_shapes(torch, group, points, scalars, counts)
    ws = _combine_workspace(torch, "combine_points", group, n, k, dev)
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    term_status = torch.empty((n, k, 2), dtype=torch.int32, device=dev) if want_term_status else None
    rc = lib().blsw_combine_points_batch(group, points.data_ptr(), scalars.data_ptr(), counts.data_ptr() if counts is not None else None, k, n, out.data_ptr(),
                                         status.data_ptr(), term_status.data_ptr() if want_term_status else None, ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_combine_points_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return (out, status, term_status) if want_term_status else (out, status)


def msm_points(group, points, scalars, counts=None, window_bits=0):
    """combine_points for LONG lists, by the bucket method (blsw_msm_points_batch, include/blsw.h): the same arguments, and for every input both
    accept the same (sum, status) byte for byte; k up to 2^24 terms per list; no term statuses. window_bits 0 is the library's choice from k, 1 .. 16
    are taken as given. combine_points pays a ladder per term and sums a list on one lane; this pays about ceil(255 / window_bits) mixed additions
    per term and a fixed tail per list: measured on ONE list the ladder wins up to 64 terms and the buckets from 256 on (65 536 terms: 48 ms in G1, 92 ms
    in G2 against 1.7 s and 4.9 s); many short lists belong there, one or a few long lists here (tools/msm_rate.py, profiles/msm_rate.txt).
    PUBLIC scalars only. -> (sum [n, 48 | 96] uint8, status [n] int32)."""
    torch = _require_cuda()
    n, k, nbytes, dev = _combine_shapes(torch, group, points, scalars, counts)
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_msm_workspace_bytes(group, n, k, window_bits, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_msm_workspace_bytes failed: %d" % rc)
    check_capacity(dev, "msm_points (n = %d, %d terms each, window_bits %d)" % (n, k, window_bits), wb.value)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    rc = lib().blsw_msm_points_batch(group, points.data_ptr(), scalars.data_ptr(), counts.data_ptr() if counts is not None else None, k, n, window_bits, out.data_ptr(),
                                     status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_msm_points_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return out, status


def lagrange_coefficients(ids, counts=None):
    """Lagrange coefficients at 0 (blsw_lagrange_batch): ids [n, k, 32] uint8 cuda, little-endian elements of Fr, non-zero and distinct within a list's
    used ids -> (coeff [n, k, 32] uint8, status [n] int32: ST_OK, ST_BAD_INDEX, ST_IDENTITY (no id), ST_BAD_ENCODING (an id >= r) or ST_BAD_ID). Rows
    beyond a count and every row of a failing list are zeros."""
    torch = _require_cuda()
    n, k = ids.shape[0], ids.shape[1]
    assert ids.shape == (n, k, 32) and ids.dtype == torch.uint8 and ids.is_contiguous() and n > 0 and k > 0
    dev = ids.device
    if counts is not None:
        assert counts.shape == (n,) and counts.element_size() == 4 and not counts.is_floating_point() and counts.is_contiguous() and counts.device == dev
    coeff = torch.empty((n, k, 32), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    rc = lib().blsw_lagrange_batch(ids.data_ptr(), counts.data_ptr() if counts is not None else None, k, n, coeff.data_ptr(), status.data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_lagrange_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return coeff, status


def recover_points(group, ids, points, counts=None):
    """sum_j lambda_j(ids) * P_j (blsw_recover_points_batch): threshold recovery from shares at `ids` -> (sum [n, 48 | 96] uint8, status [n] int32)"""
    torch = _require_cuda()
    n, k, nbytes, dev = _combine_shapes(torch, group, points, ids, counts)
    ws = _combine_workspace(torch, "recover_points", group, n, k, dev)
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    rc = lib().blsw_recover_points_batch(group, points.data_ptr(), ids.data_ptr(), counts.data_ptr() if counts is not None else None, k, n, out.data_ptr(), status.data_ptr(),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_recover_points_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return out, status


def recover_signature(ids, sig96, counts=None):
    """the group signature from partial signatures [n, k, 96] of the shares at ids [n, k, 32]"""
    return recover_points(2, ids, sig96, counts)


def recover_public_key(ids, pk48, counts=None):
    """the group public key from share keys [n, k, 48] of the shares at ids [n, k, 32]"""
    return recover_points(1, ids, pk48, counts)


_VERIFY_WS = {}


def verify_batch(pk48, msg, sig96, want_status=False, dst=None):
    """BLS::verify (bls.rs:427-458) for a batch as VALUES (blsw_verify_batch: the native algorithm — decode with subgroup checks, hash to G2, a two-pair
    Miller loop over projective lines, final exponentiation — no circuit): uint8 cuda tensors pk48 [n, 48], msg [n, msg_len], sig96 [n, 96] ->
    int32 [n] verdicts (1 / 0; every Err of the reference's verify counts as false), optionally with the decode statuses [n, 2].
    dst (here and on every value function that takes it): None = the library's tag DST_DEFAULT through the plain entry; bytes of 1 .. 255 = the
    domain separation tag of hash_to_curve, through the entry's _dst form (include/blsw.h) — the same workspace, another hash kernel."""
    torch = _require_cuda()
    n, msg_len = pk48.shape[0], msg.shape[1]
    assert pk48.shape == (n, 48) and sig96.shape == (n, 96) and msg.shape[0] == n and pk48.is_contiguous() and sig96.is_contiguous() and msg.is_contiguous()
    dev = pk48.device
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_verify_workspace_bytes(n, msg_len, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_verify_workspace_bytes failed: %d" % rc)
    key = (str(dev), wb.value)
    ws = _VERIFY_WS.get(key)
    if ws is None:  # one workspace per (device, size): repeated calls of one batch shape (a verifier's loop) do not reallocate
        _VERIFY_WS.clear()
        ws = _VERIFY_WS[key] = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    rc = _dst_entry("blsw_verify_batch", dst)(pk48.data_ptr(), sig96.data_ptr(), msg.data_ptr() if msg_len else None, msg_len, n, res.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_verify_batch failed: %d" % rc)
    return (res, status) if want_status else res


def _header_define(name):
    """an integer #define of include/blsw.h (the header is the one place such a number is written)"""
    import re

    text = open(os.path.join(HERE, "..", "include", "blsw.h")).read()
    return int(re.search(r"^#define\s+%s\s+(\w+)" % name, text, flags=re.M).group(1), 0)


VERIFY_GROUPS_CHUNK = _header_define("BLSW_VGROUP_CHUNK")  # pairs one six-lane team folds with shared squarings


def _group_scalars(torch, n, dev):
    """n fresh 64-bit coefficients from the operating system's generator, none of them zero"""
    import secrets

    import numpy as np

    r = np.frombuffer(secrets.token_bytes(8 * n), dtype=np.uint64).copy()
    r[r == 0] = 1
    return torch.from_numpy(r.view(np.int64)).to(dev)


def _msg_index_rows(torch, msg_index, n, n_msgs):
    """msg_index [n] of 32-bit integers (int32 storage of the uint32 indices) -> (int64 rows clamped into the table, bool: the index is beyond it)"""
    assert msg_index.shape == (n,) and msg_index.element_size() == 4 and not msg_index.is_floating_point() and msg_index.is_contiguous()
    rows = msg_index.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    beyond = rows >= n_msgs
    return torch.where(beyond, torch.zeros_like(rows), rows), beyond


def verify_groups(pk48, msg, sig96, group=64, scalars=None, want_status=False, dst=None, msg_index=None, want_runs=False):
    """Batch verification of GROUPS of triples with random coefficients (blsw_verify_groups_batch, include/blsw.h): group j is instances
    [j * group, min(n, (j + 1) * group)) and its verdict is 1 iff every instance decodes (both statuses OK), every coefficient is non-zero and
    prod_i e(r_i pk_i, H(m_i)) * e(-g1, sum_i r_i sig_i) == 1 — one final exponentiation per group instead of one per triple. uint8 cuda tensors as
    verify_batch -> int32 [ceil(n / group)], optionally with the decode statuses [n, 2].
    scalars: None draws n 64-bit coefficients from secrets.token_bytes on the host (zeros replaced by 1); a given int64 / uint64 cuda tensor [n] is
    used as is — predictable coefficients are NOT sound (include/blsw.h, P4). The workspace is allocated per call (the caching allocator keeps it).
    msg_index: None is the call above. A cuda tensor [n] of 32-bit integers makes msg the TABLE [n_msgs, msg_len] and instance i sign row
    msg_index[i] (blsw_verify_groups_shared_batch): one hash per row, one pair per run of equal adjacent indices of a group — sort each group by
    index. An index beyond the table is ST_BAD_INDEX in status[i, 0] and fails its group. want_runs (with an index) appends the runs per group,
    int32 [ceil(n / group)], after the status."""
    torch = _require_cuda()
    n, msg_len = pk48.shape[0], msg.shape[1]
    assert pk48.shape == (n, 48) and sig96.shape == (n, 96) and (msg.shape[0] == n or msg_index is not None) and pk48.is_contiguous() and sig96.is_contiguous() and msg.is_contiguous()
    dev = pk48.device
    if msg_index is None and want_runs:
        raise ValueError("want_runs needs msg_index: without a message table there are no runs")
    if scalars is None:
        scalars = _group_scalars(torch, n, dev)
    assert scalars.shape == (n,) and scalars.element_size() == 8 and not scalars.is_floating_point() and scalars.is_contiguous() and scalars.device == dev
    wb = ctypes.c_uint64(0)
    if msg_index is not None:
        n_msgs = msg.shape[0]
        assert msg_index.shape == (n,) and msg_index.element_size() == 4 and not msg_index.is_floating_point() and msg_index.is_contiguous() and msg_index.device == dev
        rc = lib().blsw_verify_groups_shared_workspace_bytes(n, n_msgs, msg_len, group, ctypes.byref(wb))
        if rc:
            raise BlswError("blsw_verify_groups_shared_workspace_bytes failed: %d" % rc)
        ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
        res = torch.empty((n + group - 1) // group, dtype=torch.int32, device=dev)
        runs = torch.empty((n + group - 1) // group, dtype=torch.int32, device=dev) if want_runs else None
        status = torch.empty((n, 2), dtype=torch.int32, device=dev)
        tag = _dst_struct(dst) if dst is not None else None
        rc = lib().blsw_verify_groups_shared_batch(pk48.data_ptr(), sig96.data_ptr(), msg.data_ptr() if msg_len else None, msg_len, n_msgs, msg_index.data_ptr(), n, scalars.data_ptr(),
                                                   group, ctypes.byref(tag) if tag is not None else None, res.data_ptr(), runs.data_ptr() if want_runs else None, status.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            raise BlswError("blsw_verify_groups_shared_batch failed: %d" % rc)
        extra = ([status] if want_status else []) + ([runs] if want_runs else [])
        return (res, *extra) if extra else res
    rc = lib().blsw_verify_groups_workspace_bytes(n, msg_len, group, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_verify_groups_workspace_bytes failed: %d" % rc)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty((n + group - 1) // group, dtype=torch.int32, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    rc = _dst_entry("blsw_verify_groups_batch", dst)(pk48.data_ptr(), sig96.data_ptr(), msg.data_ptr() if msg_len else None, msg_len, n, scalars.data_ptr(), group, res.data_ptr(),
                                        status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_verify_groups_batch failed: %d" % rc)
    return (res, status) if want_status else res


def verify_batch_grouped(pk48, msg, sig96, group=64, scalars=None, want_status=False, dst=None, msg_index=None, want_runs=False):
    """verify_batch through verify_groups: int32 [n] with the meaning of verify_batch. The instances of passing groups are 1; the instances of failing
    groups are gathered, put through verify_batch and scattered back. ONE host synchronisation, to learn which groups failed. A batch in which most
    groups hold a bad instance is slower this way than verify_batch: it pays for the groups and then for nearly the whole batch again.
    msg_index / want_runs: verify_groups' message table; the failing groups' instances are re-checked on their gathered rows, and an instance whose
    index lies beyond the table is 0."""
    torch = _require_cuda()
    n = pk48.shape[0]
    if msg_index is None:
        if want_runs:
            raise ValueError("want_runs needs msg_index: without a message table there are no runs")
        gres, status = verify_groups(pk48, msg, sig96, group=group, scalars=scalars, want_status=True, dst=dst)
        runs = None
    else:
        gres, status, runs = verify_groups(pk48, msg, sig96, group=group, scalars=scalars, want_status=True, dst=dst, msg_index=msg_index, want_runs=True)
    res = gres.repeat_interleave(group)[:n].contiguous()
    bad = torch.nonzero(res == 0).flatten()  # the synchronisation
    if bad.numel():
        if msg_index is None:
            res[bad] = verify_batch(pk48[bad].contiguous(), msg[bad].contiguous(), sig96[bad].contiguous(), dst=dst)
        else:
            rows, beyond = _msg_index_rows(torch, msg_index, n, msg.shape[0])
            sub = verify_batch(pk48[bad].contiguous(), msg[rows[bad]].contiguous(), sig96[bad].contiguous(), dst=dst)
            res[bad] = torch.where(beyond[bad], torch.zeros_like(sub), sub)
    extra = ([status] if want_status else []) + ([runs] if want_runs else [])
    return (res, *extra) if extra else res


VERIFY_PAIRS_CHUNK = _header_define("BLSW_VPAIRS_CHUNK")  # pairs of one instance that one six-lane team folds with shared squarings


def verify_pairs(pks48, msgs, sig96, counts=None, want_status=False, want_key_status=False, dst=None):
    """AggregateVerify as values (blsw_verify_pairs_batch, include/blsw.h): ONE aggregate signature per instance over K (key, message) pairs with their
    own messages, e(-g1, sig) * prod_j e(pk_j, H(m_j)) == 1 — every key decoded with its subgroup check and refused when it is the identity, one final
    exponentiation per instance. uint8 cuda tensors pks48 [n, K, 48], msgs [n, K, msg_len], sig96 [n, 96]; counts: None (every instance uses all K
    pairs) or an int32 / uint32 cuda tensor [n] — instance i uses its FIRST counts[i] pairs, which is how ragged lists travel padded to the longest.
    -> int32 [n] verdicts (1 / 0; a count of 0 or beyond K, a key or signature that does not decode and an identity key are false), or a tuple of
    them followed by what was asked for, in this order: status [n, 2] int32 ([i, 0] of the instance's keys and count, [i, 1] of the signature),
    key_status [n, K] int32 of every key, used or not. The workspace is allocated per call (the caching allocator keeps it) after check_capacity: its
    dominant term is 19.6 KB of lines per pair."""
    torch = _require_cuda()
    n, K, msg_len = pks48.shape[0], pks48.shape[1], msgs.shape[2]
    assert pks48.shape == (n, K, 48) and msgs.shape == (n, K, msg_len) and sig96.shape == (n, 96)
    assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (pks48, msgs, sig96))
    dev = pks48.device
    if counts is not None:
        assert counts.shape == (n,) and counts.element_size() == 4 and not counts.is_floating_point() and counts.is_contiguous() and counts.device == dev
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_verify_pairs_workspace_bytes(n, msg_len, K, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_verify_pairs_workspace_bytes failed: %d" % rc)
    check_capacity(dev, "verify_pairs (n = %d, %d pairs)" % (n, K), wb.value)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    key_status = torch.empty((n, K), dtype=torch.int32, device=dev) if want_key_status else None
    rc = _dst_entry("blsw_verify_pairs_batch", dst)(pks48.data_ptr(), msgs.data_ptr() if msg_len else None, msg_len, K, counts.data_ptr() if counts is not None else None, sig96.data_ptr(), n,
                                       res.data_ptr(), status.data_ptr(), key_status.data_ptr() if want_key_status else None, ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_verify_pairs_batch failed: %d" % rc)
    extra = ([status] if want_status else []) + ([key_status] if want_key_status else [])
    return (res, *extra) if extra else res


COMMITTEE_LANES = _header_define("BLSW_COMMITTEE_LANES")  # lanes that share one instance's key sum


def committee_verify(pks48, bitmap, msg, sig96, group=0, scalars=None, want_status=False, want_count=False, want_aggregate=False, dst=None):
    """fast_aggregate_verify as values over ONE committee and n bitmaps (blsw_committee_verify_batch, include/blsw.h): uint8 cuda tensors pks48
    [K, 48] (the committee, given once), bitmap [n, K] (a non-zero byte selects the key), msg [n, msg_len], sig96 [n, 96]. The committee is decoded
    once per call and every instance sums its selected keys with COMMITTEE_LANES lanes.
    group == 0 -> int32 [n]: the verdict of fast_aggregate_verify_batch on the selected keys (an empty selection, a selected key that does not
    decode and an identity aggregate are false). group >= 1 -> int32 [ceil(n / group)]: verify_groups' statement over the aggregated keys; scalars
    None draws coefficients as verify_groups does.
    Returns the verdicts, or a tuple of them followed by what was asked for, in this order: (status [n, 2] int32 — [i, 0] of the aggregate key,
    [i, 1] of the signature —, key_status [K] int32), count [n] (int32 storage of the uint32 counts), aggregate [n, 48] uint8. The workspace is
    allocated per call (the caching allocator keeps it)."""
    torch = _require_cuda()
    K, n, msg_len = pks48.shape[0], bitmap.shape[0], msg.shape[1]
    assert pks48.shape == (K, 48) and bitmap.shape == (n, K) and sig96.shape == (n, 96) and msg.shape[0] == n
    assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (pks48, bitmap, msg, sig96))
    dev = pks48.device
    if group and scalars is None:
        scalars = _group_scalars(torch, n, dev)
    if scalars is not None:
        assert scalars.shape == (n,) and scalars.element_size() == 8 and not scalars.is_floating_point() and scalars.is_contiguous() and scalars.device == dev
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_committee_verify_workspace_bytes(n, msg_len, K, group, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_committee_verify_workspace_bytes failed: %d" % rc)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty((n + group - 1) // group if group else n, dtype=torch.int32, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    key_status = torch.empty(K, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev) if want_count else None
    agg = torch.empty((n, 48), dtype=torch.uint8, device=dev) if want_aggregate else None
    rc = _dst_entry("blsw_committee_verify_batch", dst)(pks48.data_ptr(), K, bitmap.data_ptr(), sig96.data_ptr(), msg.data_ptr() if msg_len else None, msg_len, n,
                                           scalars.data_ptr() if scalars is not None else None, group, res.data_ptr(), count.data_ptr() if want_count else None,
                                           status.data_ptr(), key_status.data_ptr(), agg.data_ptr() if want_aggregate else None, ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_committee_verify_batch failed: %d" % rc)
    extra = ([(status, key_status)] if want_status else []) + ([count] if want_count else []) + ([agg] if want_aggregate else [])
    return (res, *extra) if extra else res


def committee_verify_grouped(pks48, bitmap, msg, sig96, group=64, scalars=None, want_status=False, dst=None):
    """committee_verify(group=0)'s per-instance verdicts through the grouped form: the instances of passing groups are 1; the instances of failing
    groups are gathered, put through committee_verify(group=0) and scattered back. ONE host synchronisation, to learn which groups failed, like
    verify_batch_grouped — and like it slower than the plain call when most groups hold a bad instance."""
    torch = _require_cuda()
    n = bitmap.shape[0]
    gres, st = committee_verify(pks48, bitmap, msg, sig96, group=group, scalars=scalars, want_status=True, dst=dst)
    res = gres.repeat_interleave(group)[:n].contiguous()
    bad = torch.nonzero(res == 0).flatten()  # the synchronisation
    if bad.numel():
        res[bad] = committee_verify(pks48, bitmap[bad].contiguous(), msg[bad].contiguous(), sig96[bad].contiguous(), dst=dst)
    return (res, st) if want_status else res


REGISTRY_LANES = _header_define("BLSW_REGISTRY_LANES")  # lanes that share one set's key sum
ST_BAD_INDEX = _header_define("BLSW_ST_BAD_INDEX")


class KeyRegistry:
    """A resident registry of public keys (blsw_registry_*, include/blsw.h): room for `capacity` keys (1 .. 2^24) in a device buffer this object
    owns; append() decodes compressed keys ONCE, with the subgroup check, on the current stream of `device`, and registry_verify sums index lists
    over them. A verify call must be ordered behind the appends it relies on (the same stream does that); the object is not thread-safe."""

    def __init__(self, capacity, device=None):
        torch = _require_cuda()
        self.capacity = int(capacity)
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if self.device.index is None:  # "cuda": the current device, with its index, so that it compares equal to the tensors' devices
            self.device = torch.device("cuda", torch.cuda.current_device())
        b = ctypes.c_uint64(0)
        rc = lib().blsw_registry_bytes(self.capacity, ctypes.byref(b))
        if rc:
            raise BlswError("blsw_registry_bytes failed: %d" % rc)
        self.buffer = torch.empty(b.value, dtype=torch.uint8, device=self.device)  # the allocator's blocks are 512-byte aligned
        self._r = ctypes.c_void_p()
        rc = lib().blsw_registry_create(ctypes.byref(self._r), self.capacity, self.device.index, self.buffer.data_ptr(), self.buffer.numel())
        if rc:
            self._r = None
            raise BlswError("blsw_registry_create failed: %d" % rc)
        ptr = ctypes.c_void_p()
        rc = lib().blsw_registry_key_status(self._r, ctypes.byref(ptr))
        off = (ptr.value or 0) - self.buffer.data_ptr()
        if rc or off < 0 or off + 4 * self.capacity > self.buffer.numel():
            raise BlswError("blsw_registry_key_status failed: %d" % rc)
        self._status = self.buffer[off:off + 4 * self.capacity].view(torch.int32)

    def append(self, pks48):
        """uint8 cuda tensor [m, 48] of compressed keys -> they become keys [size, size + m); returns the new size"""
        torch = _require_cuda()
        assert pks48.dim() == 2 and pks48.shape[1] == 48 and pks48.dtype == torch.uint8 and pks48.is_contiguous() and pks48.device == self.device
        rc = lib().blsw_registry_append(self._r, pks48.data_ptr(), pks48.shape[0], torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            raise BlswError("blsw_registry_append failed: %d" % rc)
        return self.size

    @property
    def size(self):
        n = ctypes.c_uint32(0)
        rc = lib().blsw_registry_size(self._r, ctypes.byref(n))
        if rc:
            raise BlswError("blsw_registry_size failed: %d" % rc)
        return n.value

    def key_status(self):
        """int32 [size] view of the keys' statuses, defined once the appends have run on their stream"""
        return self._status[:self.size]

    def msm(self, indices, offsets, scalars, window_bits=0):
        """sum_p s_p * key[index_p] per index list, by the bucket method (blsw_registry_msm_batch, include/blsw.h): list i is
        indices[offsets[i]:offsets[i + 1]] as in registry_verify, scalars [n_indices, 32] uint8 little-endian below r, PUBLIC, one per position.
        -> (sum48 [n, 48] uint8 — zeros for a failing list, the infinity encoding for an identity sum —, status [n] int32: ST_BAD_INDEX for bad
        offsets or an index >= size, ST_IDENTITY for an empty list, a bad key's status, ST_BAD_ENCODING for a scalar >= r, each at the earliest bad
        position). For an OK list the bytes are combine_points' on the gathered keys; measured on one list it is below combine_points at every
        length from 16 terms on (it decodes nothing), 66 ms against 1.7 s at 65 536. Must be ordered behind the appends it relies on (the same stream does that)."""
        torch = _require_cuda()
        n, n_indices, dev = offsets.shape[0] - 1, indices.shape[0], self.device
        assert indices.dim() == 1 and offsets.dim() == 1 and n >= 1 and scalars.shape == (n_indices, 32) and scalars.dtype == torch.uint8
        assert indices.element_size() == 4 and offsets.element_size() == 8 and not indices.is_floating_point() and not offsets.is_floating_point()
        assert all(t.is_contiguous() and t.device == dev for t in (indices, offsets, scalars))
        wb = ctypes.c_uint64(0)
        rc = lib().blsw_registry_msm_workspace_bytes(n, n_indices, window_bits, ctypes.byref(wb))
        if rc:
            raise BlswError("blsw_registry_msm_workspace_bytes failed: %d" % rc)
        check_capacity(dev, "KeyRegistry.msm (n = %d, %d indices, window_bits %d)" % (n, n_indices, window_bits), wb.value)
        ws = torch.empty(max(wb.value, 256), dtype=torch.uint8, device=dev)
        out = torch.empty((n, 48), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        rc = lib().blsw_registry_msm_batch(self._r, indices.data_ptr() if n_indices else None, n_indices, offsets.data_ptr(), scalars.data_ptr() if n_indices else None, n,
                                           window_bits, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            raise BlswError("blsw_registry_msm_batch failed: %d" % rc)
        torch.cuda.synchronize(dev)
        return out, status

    def close(self):
        if getattr(self, "_r", None):
            lib().blsw_registry_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def registry_verify(registry, indices, offsets, msg, sig96, group=0, scalars=None, want_status=False, want_aggregate=False, dst=None, msg_index=None, want_runs=False):
    """fast_aggregate_verify as values over a KeyRegistry and n index lists (blsw_registry_verify_batch, include/blsw.h): set i is
    indices[offsets[i]:offsets[i + 1]] — indices a cuda tensor [n_indices] of 32-bit integers (int32 storage of the uint32 indices), offsets [n + 1]
    of 64-bit integers; uint8 cuda tensors msg [n, msg_len], sig96 [n, 96]. A repeated index is added as often as it occurs.
    group == 0 -> int32 [n]: the verdict of fast_aggregate_verify_batch on the gathered keys (an empty list, a bad entry and an identity sum are
    false). group >= 1 -> int32 [ceil(n / group)]: verify_groups' statement over the sets' sums; scalars None draws coefficients as verify_groups does.
    Returns the verdicts, or a tuple of them followed by what was asked for, in this order: status [n, 2] int32 ([i, 0] of the set's key —
    ST_BAD_INDEX for bad offsets or an index >= registry.size —, [i, 1] of the signature), aggregate [n, 48] uint8, runs.
    msg_index: None is the call above. A cuda tensor [n] of 32-bit integers makes msg the TABLE [n_msgs, msg_len] and set i sign row msg_index[i].
    group >= 1 runs blsw_registry_verify_shared_batch (one hash per row, one pair per run of equal adjacent indices of a group: sort each group by
    index), and want_runs appends the runs per group, int32 [ceil(n / group)]. group == 0 gathers msg[msg_index] and calls the plain entry. In both
    an index beyond the table is ST_BAD_INDEX in status[i, 0] and false."""
    torch = _require_cuda()
    if msg_index is None and want_runs:
        raise ValueError("want_runs needs msg_index: without a message table there are no runs")
    if msg_index is not None:
        return _registry_verify_shared(torch, registry, indices, offsets, msg, sig96, group, scalars, want_status, want_aggregate, dst, msg_index, want_runs)
    n, msg_len, n_indices = msg.shape[0], msg.shape[1], indices.shape[0]
    assert indices.dim() == 1 and offsets.shape == (n + 1,) and sig96.shape == (n, 96)
    assert indices.element_size() == 4 and offsets.element_size() == 8 and not indices.is_floating_point() and not offsets.is_floating_point()
    assert all(t.is_contiguous() and t.device == registry.device for t in (indices, offsets, msg, sig96)) and msg.dtype == torch.uint8 and sig96.dtype == torch.uint8
    dev = registry.device
    if group and scalars is None:
        scalars = _group_scalars(torch, n, dev)
    if scalars is not None:
        assert scalars.shape == (n,) and scalars.element_size() == 8 and not scalars.is_floating_point() and scalars.is_contiguous() and scalars.device == dev
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_registry_verify_workspace_bytes(n, msg_len, group, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_registry_verify_workspace_bytes failed: %d" % rc)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty((n + group - 1) // group if group else n, dtype=torch.int32, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    agg = torch.empty((n, 48), dtype=torch.uint8, device=dev) if want_aggregate else None
    rc = _dst_entry("blsw_registry_verify_batch", dst)(registry._r, indices.data_ptr() if n_indices else None, n_indices, offsets.data_ptr(), sig96.data_ptr(),
                                          msg.data_ptr() if msg_len else None, msg_len, n, scalars.data_ptr() if scalars is not None else None, group, res.data_ptr(),
                                          status.data_ptr(), agg.data_ptr() if want_aggregate else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_registry_verify_batch failed: %d" % rc)
    extra = ([status] if want_status else []) + ([agg] if want_aggregate else [])
    return (res, *extra) if extra else res


def _registry_verify_shared(torch, registry, indices, offsets, msg, sig96, group, scalars, want_status, want_aggregate, dst, msg_index, want_runs):
    """registry_verify over a message table (its docstring has the rules)"""
    n, n_msgs, msg_len, n_indices, dev = sig96.shape[0], msg.shape[0], msg.shape[1], indices.shape[0], registry.device
    assert msg_index.shape == (n,) and msg_index.element_size() == 4 and not msg_index.is_floating_point() and msg_index.is_contiguous() and msg_index.device == dev
    if group == 0:  # nothing is shared per set: a gather and the plain entry, the bad-index rule placed in front here
        if want_runs:
            raise ValueError("want_runs needs group >= 1: the per-set form has no runs")
        rows, beyond = _msg_index_rows(torch, msg_index, n, n_msgs)
        out = registry_verify(registry, indices, offsets, msg[rows].contiguous(), sig96, want_status=True, want_aggregate=want_aggregate, dst=dst)
        res, status = out[0], out[1]
        res = torch.where(beyond, torch.zeros_like(res), res)
        status[:, 0] = torch.where(beyond, torch.full_like(status[:, 0], ST_BAD_INDEX), status[:, 0])
        extra = ([status] if want_status else []) + ([out[2]] if want_aggregate else [])
        return (res, *extra) if extra else res
    assert indices.dim() == 1 and offsets.shape == (n + 1,) and sig96.shape == (n, 96)
    assert indices.element_size() == 4 and offsets.element_size() == 8 and not indices.is_floating_point() and not offsets.is_floating_point()
    assert all(t.is_contiguous() and t.device == dev for t in (indices, offsets, msg, sig96)) and msg.dtype == torch.uint8 and sig96.dtype == torch.uint8
    if scalars is None:
        scalars = _group_scalars(torch, n, dev)
    assert scalars.shape == (n,) and scalars.element_size() == 8 and not scalars.is_floating_point() and scalars.is_contiguous() and scalars.device == dev
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_registry_verify_shared_workspace_bytes(n, n_msgs, msg_len, group, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_registry_verify_shared_workspace_bytes failed: %d" % rc)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    n_groups = (n + group - 1) // group
    res = torch.empty(n_groups, dtype=torch.int32, device=dev)
    runs = torch.empty(n_groups, dtype=torch.int32, device=dev) if want_runs else None
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    agg = torch.empty((n, 48), dtype=torch.uint8, device=dev) if want_aggregate else None
    tag = _dst_struct(dst) if dst is not None else None
    rc = lib().blsw_registry_verify_shared_batch(registry._r, indices.data_ptr() if n_indices else None, n_indices, offsets.data_ptr(), sig96.data_ptr(),
                                                 msg.data_ptr() if msg_len else None, msg_len, n_msgs, msg_index.data_ptr(), n, scalars.data_ptr(), group,
                                                 ctypes.byref(tag) if tag is not None else None, res.data_ptr(), runs.data_ptr() if want_runs else None, status.data_ptr(),
                                                 agg.data_ptr() if want_aggregate else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_registry_verify_shared_batch failed: %d" % rc)
    extra = ([status] if want_status else []) + ([agg] if want_aggregate else []) + ([runs] if want_runs else [])
    return (res, *extra) if extra else res


def registry_verify_grouped(registry, indices, offsets, msg, sig96, group=64, scalars=None, want_status=False, dst=None, msg_index=None, want_runs=False):
    """registry_verify(group=0)'s per-set verdicts through the grouped form: the sets of passing groups are 1; the sets of failing groups are
    re-checked with the per-set form and scattered back. CSR is one run of n + 1 offsets and the failing sets' lists are not adjacent, so their
    entries are gathered into an index list of their own. ONE host synchronisation: the group verdicts and the n + 1 offsets come to the host in a
    single transfer, and the gather positions are laid out there. Like committee_verify_grouped it is slower than the plain call when most groups
    fail."""
    torch = _require_cuda()
    import numpy as np

    n, dev = sig96.shape[0], msg.device
    runs = None
    if msg_index is None:
        if want_runs:
            raise ValueError("want_runs needs msg_index: without a message table there are no runs")
        gres, st = registry_verify(registry, indices, offsets, msg, sig96, group=group, scalars=scalars, want_status=True, dst=dst)
    else:  # the failing groups' sets are re-checked on their gathered rows; a set whose index lies beyond the table stays 0
        gres, st, runs = registry_verify(registry, indices, offsets, msg, sig96, group=group, scalars=scalars, want_status=True, dst=dst, msg_index=msg_index, want_runs=True)
    res = gres.repeat_interleave(group)[:n].contiguous()
    host = torch.cat([res.to(torch.int64), offsets.view(torch.int64)]).cpu().numpy()  # the synchronisation
    bad = np.flatnonzero(host[:n] == 0)
    if len(bad):
        # A set whose offsets are bad becomes the empty list: false again (the statuses returned are the first call's), and nothing of it is read.
        off = host[n:]  # int64: an offset of 2^63 or more is negative here, and bad
        lo, hi = off[bad], off[bad + 1]
        ok = (lo >= 0) & (hi >= lo) & (hi <= indices.shape[0])
        ln = np.where(ok, hi - lo, 0)
        ends = np.cumsum(ln)
        pos = np.arange(ends[-1], dtype=np.int64) + np.repeat(lo - (ends - ln), ln)
        sub_idx = indices[torch.from_numpy(pos).to(dev)].contiguous()
        sub_off = torch.from_numpy(np.concatenate([np.zeros(1, np.int64), ends])).to(dev)
        bad_t = torch.from_numpy(bad).to(dev)
        if msg_index is None:
            res[bad_t] = registry_verify(registry, sub_idx, sub_off, msg[bad_t].contiguous(), sig96[bad_t].contiguous(), dst=dst)
        else:
            res[bad_t] = registry_verify(registry, sub_idx, sub_off, msg, sig96[bad_t].contiguous(), dst=dst, msg_index=msg_index[bad_t].contiguous())
    extra = ([st] if want_status else []) + ([runs] if want_runs else [])
    return (res, *extra) if extra else res


def fast_aggregate_verify_batch(pks48, msg, sig96):
    """tests/tests.rs:296-334: n instances of k compressed keys each signing ONE message: PublicKey::aggregate (blsw_aggregate_points_batch), then
    BLS::verify on the aggregate (blsw_verify_batch). A key that does not decode, an empty list or an identity aggregate is false. -> int32 [n]
    For ONE committee and a bitmap per instance (lists of different lengths over the same keys) use committee_verify: it decodes the keys once."""
    torch = _require_cuda()
    n = pks48.shape[0]
    if pks48.shape[1] == 0:
        return torch.zeros(n, dtype=torch.int32, device=pks48.device)
    agg, st = aggregate_points(1, pks48)
    res = verify_batch(agg, msg, sig96)
    return torch.where(st == 0, res, torch.zeros_like(res))


def verify_bytes_batch(pk48, msg, sig96):
    """tests/tests.rs:239-268 semantics on the GPU in one ABI call (blsw_engine_submit_bytes): decode, run the gadget, accept iff
    both points decode to non-identity subgroup points and the in-circuit result is true. Returns a bool tensor [n]."""
    torch = _require_cuda()
    eng = WitnessEngine(pk48.shape[0], msg.shape[1], device=pk48.device)
    res = torch.empty(pk48.shape[0], dtype=torch.int32, device=pk48.device)
    eng.submit_bytes(pk48.contiguous(), sig96.contiguous(), msg.contiguous(), witness=None, result=res)
    eng.flush()
    torch.cuda.synchronize(pk48.device)
    eng.close()
    return res == 1


def layout_aggregate(msg_len, n_keys, agg_inputs=0):
    """Segment table of the aggregate_verify circuit; agg_inputs: mask of AGG_*_INPUT (blsw_layout_aggregate_inputs), 0 = every argument Witness"""
    L = blsw_layout_t()
    if agg_inputs:
        rc = lib().blsw_layout_aggregate_inputs(msg_len, n_keys, agg_inputs, ctypes.byref(L))
    else:
        rc = lib().blsw_layout_aggregate(msg_len, n_keys, ctypes.byref(L))
    if rc:
        raise BlswError("blsw_layout_aggregate failed: %d" % rc)
    return {n: getattr(L, n) for n in _LAYOUT_FIELDS}


def aggregate_verify(parameters, public_keys, bitmap, message, signature, want_witness=True):
    """BlsSignatureVerifyGadget::aggregate_verify (constraints.rs:153-167) for n instances: public_keys.xy [n, K, 12] int64,
    bitmap [n, K] uint8 (0/1) or a Boolean vector, message [n, msg_len] uint8 or a UInt8 vector, signature.xy [n, 24].
    Returns (result int32 [n], count int32 [n], witness). With an argument allocated as Input (PublicKeyVar.new_input, Boolean.new_input,
    UInt8.new_input_vec, SignatureVar.new_input) the circuit is the one of layout_aggregate(msg_len, K, mask): a direct-mode engine runs it and
    the call returns (result, count, witness, instance) with instance [n, n_instance_vars, 6] = every instance's instance_assignment.
    public_keys may be a KeySet (its K keys allocated as witnesses once, the same committee for every instance): the same circuit and vectors as
    with the keys replicated [n, K, 12], through a direct-mode engine with shared_keys; the return value follows the other arguments' modes."""
    torch = _require_cuda()
    assert isinstance(parameters, ParametersVar)
    bit_var = bitmap if isinstance(bitmap, Boolean) else Boolean(bitmap)
    msg_var = message if isinstance(message, UInt8) else UInt8(message)
    if isinstance(public_keys, KeySet):
        if parameters.mode != "Constant":
            raise BlswError("aggregate_verify with a KeySet: ParametersVar allocated as %s is not offered (Constant)" % parameters.mode)
        mask = ((AGG_BITMAP_INPUT if bit_var.mode == "Input" else 0) | (AGG_MSG_INPUT if msg_var.mode == "Input" else 0) | (AGG_SIG_INPUT if signature.mode == "Input" else 0))
        sig, bits, msg = signature.xy.contiguous(), bit_var.bits.contiguous(), msg_var.bytes.contiguous()
        n, K, msg_len = bits.shape[0], public_keys.n_keys, msg.shape[1]
        lay = layout_aggregate(msg_len, K, mask)
        eng = WitnessEngine(n, msg_len, max_steps=1, n_buffers=1, device=public_keys.device, reserve_bytes=n * lay["n_witness"] * 48 if want_witness else 0, n_keys=K,
                            agg_inputs=mask, shared_keys=1, output_form=public_keys.output_form)
        try:
            res = torch.empty(n, dtype=torch.int32, device=eng.device)
            cnt = torch.empty(n, dtype=torch.int32, device=eng.device)
            wit = eng.new_witness_tensor() if want_witness else None
            inst = eng.new_instance_tensor() if mask else None
            eng.submit_aggregate_keyset(public_keys, bits, sig, msg, witness=wit, result=res, count=cnt, instance=inst)
            eng.flush()
            torch.cuda.synchronize(eng.device)
        finally:
            eng.close()
        return (res, cnt, wit, inst) if mask else (res, cnt, wit)
    mask = ((AGG_KEYS_INPUT if public_keys.mode == "Input" else 0) | (AGG_BITMAP_INPUT if bit_var.mode == "Input" else 0) |
            (AGG_MSG_INPUT if msg_var.mode == "Input" else 0) | (AGG_SIG_INPUT if signature.mode == "Input" else 0))
    pks, sig, bitmap, message = public_keys.xy.contiguous(), signature.xy.contiguous(), bit_var.bits.contiguous(), msg_var.bytes.contiguous()
    n, K = pks.shape[0], pks.shape[1]
    assert K >= 1 and bitmap.shape == (n, K)  # constraints.rs:160-162: equal lengths, at least one key
    msg_len = message.shape[1]
    if mask:
        if parameters.mode != "Constant":
            raise BlswError("aggregate_verify with Input arguments: ParametersVar allocated as %s is not offered (Constant)" % parameters.mode)
        assert sig.shape == (n, 24) and message.shape[0] == n
        lay = layout_aggregate(msg_len, K, mask)
        eng = WitnessEngine(n, msg_len, max_steps=1, n_buffers=1, device=pks.device, reserve_bytes=n * lay["n_witness"] * 48 if want_witness else 0, n_keys=K,
                            agg_inputs=mask)
        try:
            res = torch.empty(n, dtype=torch.int32, device=pks.device)
            cnt = torch.empty(n, dtype=torch.int32, device=pks.device)
            wit = eng.new_witness_tensor() if want_witness else None
            inst = eng.new_instance_tensor()
            eng.submit_aggregate(pks, bitmap, sig, message, witness=wit, result=res, count=cnt, instance=inst)
            eng.flush()
            torch.cuda.synchronize(pks.device)
        finally:
            eng.close()
        return res, cnt, wit, inst
    lay = layout_aggregate(msg_len, K)
    wb = ctypes.c_uint64(0)
    lib().blsw_aggregate_workspace_bytes(n, msg_len, K, ctypes.byref(wb))
    dev = pks.device
    check_capacity(dev, "aggregate_verify (n = %d, %d keys)" % (n, K), wb.value, n * lay["n_witness"] * 48 if want_witness else 0)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    wit = torch.empty((n, lay["n_witness"], 6), dtype=torch.int64, device=dev) if want_witness else None
    assert sig.shape == (n, 24) and message.shape[0] == n
    rc = lib().blsw_aggregate_verify_batch(pks.data_ptr(), bitmap.data_ptr(), K, sig.data_ptr(), message.data_ptr(), msg_len, n,
                                           wit.data_ptr() if wit is not None else None, lay["n_witness"], res.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                           ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_aggregate_verify_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return res, cnt, wit


def matrices(msg_len=32, n_keys=0, n_pairs=1, params_mode=0, pk_mode=0, sig_mode=0, msg_mode=0, agg_inputs=0, multi_inputs=0):
    """Constraint matrices of a circuit shape (host only; blsw_matrices_info + blsw_matrices_fill): the R1CS an arkworks prover
    takes next to the witness vectors, in ConstraintMatrices shape. Returns dict(n_constraints, n_instance_vars, n_witness,
    A / B / C = (row_ptr uint64 [n_constraints + 1], col uint32 [nnz], val uint64 [nnz, 6] Montgomery limbs)).
    params_mode 1 / "witness" (single-key circuit): the system of layout(msg_len, params_mode=1); msg_mode / pk_mode / sig_mode as layout();
    agg_inputs (with n_keys): the system of layout_aggregate(msg_len, n_keys, agg_inputs); multi_inputs (the N+1-pair product): the system of
    layout_multi(msg_len, n_pairs, multi_inputs)."""
    import numpy as np

    params_mode = PARAMS_MODES.get(params_mode, params_mode)
    pk_mode, sig_mode, msg_mode = IO_MODES.get(pk_mode, pk_mode), IO_MODES.get(sig_mode, sig_mode), IO_MODES.get(msg_mode, msg_mode)
    info = blsw_matrices_info_t()
    if agg_inputs and (not n_keys or n_pairs != 1 or params_mode):
        raise BlswError("agg_inputs applies to the aggregate_verify circuit (n_keys > 0)")
    agg = bool(agg_inputs) and not (msg_mode or pk_mode or sig_mode)  # the three single-key modes stay refused together with n_keys, below
    if multi_inputs and (n_keys or params_mode or agg_inputs):
        raise BlswError("multi_inputs applies to the N+1-pair product (n_keys 0, Constant parameters)")
    multi = bool(multi_inputs) and not (msg_mode or pk_mode or sig_mode)  # and together with n_pairs != 1
    if multi:
        rc = lib().blsw_matrices_info_multi_inputs(msg_len, n_pairs, multi_inputs, ctypes.byref(info))
    elif agg:
        rc = lib().blsw_matrices_info_aggregate_inputs(msg_len, n_keys, agg_inputs, ctypes.byref(info))
    elif msg_mode:  # columns: 0 = one, the message chunks, the key's and the signature's inputs, then the witnesses
        if n_keys or n_pairs != 1 or params_mode:
            raise BlswError("msg_mode applies to the single-key circuit with Constant parameters")
        rc = lib().blsw_matrices_info_inputs(msg_len, msg_mode, pk_mode, sig_mode, ctypes.byref(info))
    elif pk_mode or sig_mode:  # columns: 0 = one, 1 .. n_instance_vars - 1 = the public inputs, n_instance_vars + k = witness k
        if n_keys or n_pairs != 1 or params_mode:
            raise BlswError("pk_mode / sig_mode apply to the single-key circuit with Constant parameters")
        rc = lib().blsw_matrices_info_io(msg_len, pk_mode, sig_mode, ctypes.byref(info))
    elif params_mode:
        if n_keys or n_pairs != 1:
            raise BlswError("params_mode applies to the single-key circuit")
        rc = lib().blsw_matrices_info_params(msg_len, params_mode, ctypes.byref(info))
    else:
        rc = lib().blsw_matrices_info(msg_len, n_keys, n_pairs, ctypes.byref(info))
    if rc:
        raise BlswError("blsw_matrices_info failed: %d" % rc)
    u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    rp = [np.zeros(info.n_constraints + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(info.nnz[m], dtype=np.uint32) for m in range(3)]
    val = [np.zeros((info.nnz[m], 6), dtype=np.uint64) for m in range(3)]
    out = blsw_matrices_t()
    for m in range(3):
        out.row_ptr[m] = rp[m].ctypes.data_as(u64p)
        out.col[m] = col[m].ctypes.data_as(u32p)
        out.val[m] = val[m].ctypes.data_as(u64p)
    if multi:
        rc = lib().blsw_matrices_fill_multi_inputs(msg_len, n_pairs, multi_inputs, ctypes.byref(info), ctypes.byref(out))
    elif agg:
        rc = lib().blsw_matrices_fill_aggregate_inputs(msg_len, n_keys, agg_inputs, ctypes.byref(info), ctypes.byref(out))
    elif msg_mode:
        rc = lib().blsw_matrices_fill_inputs(msg_len, msg_mode, pk_mode, sig_mode, ctypes.byref(info), ctypes.byref(out))
    elif pk_mode or sig_mode:
        rc = lib().blsw_matrices_fill_io(msg_len, pk_mode, sig_mode, ctypes.byref(info), ctypes.byref(out))
    elif params_mode:
        rc = lib().blsw_matrices_fill_params(msg_len, params_mode, ctypes.byref(info), ctypes.byref(out))
    else:
        rc = lib().blsw_matrices_fill(msg_len, n_keys, n_pairs, ctypes.byref(info), ctypes.byref(out))
    if rc:
        raise BlswError("blsw_matrices_fill failed: %d" % rc)
    return {"n_constraints": info.n_constraints, "n_instance_vars": info.n_instance_vars, "n_witness": info.n_witness,
            "A": (rp[0], col[0], val[0]), "B": (rp[1], col[1], val[1]), "C": (rp[2], col[2], val[2])}


def _matrices_struct(mats):
    """(blsw_matrices_info_t, blsw_matrices_t) pointing into the numpy arrays of a matrices() dict (which must stay alive)"""
    import numpy as np

    info = blsw_matrices_info_t(mats["n_constraints"], mats["n_instance_vars"], mats["n_witness"])
    m = blsw_matrices_t()
    for k, name in enumerate("ABC"):
        rp, col, val = mats[name]
        assert rp.dtype == np.uint64 and col.dtype == np.uint32 and val.dtype == np.uint64 and rp.flags.c_contiguous and col.flags.c_contiguous and val.flags.c_contiguous
        info.nnz[k] = col.shape[0]
        m.row_ptr[k] = rp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        m.col[k] = col.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        m.val[k] = val.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    return info, m


def r1cs_device_bytes(mats):
    """blsw_r1cs_device_bytes: bytes of the device encoding of a matrices() dict (validates it: BlswError on a malformed CSR)"""
    info, m = _matrices_struct(mats)
    b = ctypes.c_uint64(0)
    rc = lib().blsw_r1cs_device_bytes(ctypes.byref(info), ctypes.byref(m), ctypes.byref(b))
    if rc:
        raise BlswError("blsw_r1cs_device_bytes failed: %d" % rc)
    return b.value


def r1cs_head_rows(mats, head_len):
    """blsw_r1cs_head_rows: the number of leading constraints of a matrices() dict that read nothing but column 0 and the first head_len witnesses
    (host only; validates the CSR like r1cs_device_bytes)"""
    info, m = _matrices_struct(mats)
    rows = ctypes.c_uint64(0)
    rc = lib().blsw_r1cs_head_rows(ctypes.byref(info), ctypes.byref(m), head_len, ctypes.byref(rows))
    if rc:
        raise BlswError("blsw_r1cs_head_rows failed: %d" % rc)
    return rows.value


def _pair_families(call, layout):
    assert isinstance(layout, blsw_compact_layout_multi_t)
    import numpy as np

    count = ctypes.c_uint64(0)
    rc = call(ctypes.byref(layout), 0, None, None, ctypes.byref(count))
    if rc:
        raise BlswError("blsw_r1cs_pair_families failed: %d" % rc)
    first, rows = np.zeros(max(count.value, 1), np.uint64), np.zeros(max(count.value, 1), np.uint64)
    rc = call(ctypes.byref(layout), count.value, first.ctypes.data, rows.ctypes.data, ctypes.byref(count))
    if rc:
        raise BlswError("blsw_r1cs_pair_families failed: %d" % rc)
    return [(int(f), int(r)) for f, r in zip(first[:count.value], rows[:count.value])]


def r1cs_pair_families(mats, layout):
    """blsw_r1cs_pair_families: the pair families [(first_row, rows_per_pair)] of a matrices() dict under a blsw_compact_layout_multi_t — runs of
    n_pairs consecutive blocks that are translated copies of the first, entry for entry (host only; validates the CSR like r1cs_device_bytes)"""
    info, m = _matrices_struct(mats)
    return _pair_families(lambda *a: lib().blsw_r1cs_pair_families(ctypes.byref(info), ctypes.byref(m), *a), layout)


class ConstraintChecker:
    """The constraint system of one circuit shape on the GPU (blsw_r1cs_*): arkworks' cs.is_satisfied() / cs.which_is_unsatisfied() and the
    A z, B z, C z rows, for a batch of witness vectors at once. Arguments as matrices(). Inputs are the tensors WitnessEngine writes:
    witness [n, >= n_witness, 6] int64 (a padded stride is honoured), instance [n, >= n_instance_vars, 6] (required when the circuit has
    public inputs), form 0 = Montgomery, 1 = canonical (options.output_form). The encoded matrices live in a device tensor this object
    owns; it is read-only after construction and recorded on every stream a call runs on."""

    def __init__(self, msg_len=32, n_keys=0, n_pairs=1, params_mode=0, pk_mode=0, sig_mode=0, device=None, _mats=None, msg_mode=0, agg_inputs=0, multi_inputs=0):
        torch = _require_cuda()
        self.torch = torch
        mats = _mats if _mats is not None else matrices(msg_len, n_keys, n_pairs, params_mode, pk_mode, sig_mode, msg_mode, agg_inputs, multi_inputs)
        self.n_constraints, self.n_instance_vars, self.n_witness = int(mats["n_constraints"]), int(mats["n_instance_vars"]), int(mats["n_witness"])
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda:%d" % torch.cuda.current_device())
        info, m = _matrices_struct(mats)
        b = ctypes.c_uint64(0)
        rc = lib().blsw_r1cs_device_bytes(ctypes.byref(info), ctypes.byref(m), ctypes.byref(b))
        if rc:
            raise BlswError("blsw_r1cs_device_bytes failed: %d" % rc)
        self.buffer = torch.empty(b.value, dtype=torch.uint8, device=self.device)
        self._r = ctypes.c_void_p()
        stream = torch.cuda.current_stream(self.device)
        rc = lib().blsw_r1cs_create(ctypes.byref(self._r), ctypes.byref(info), ctypes.byref(m), self.device.index, self.buffer.data_ptr(), self.buffer.numel(),
                                    stream.cuda_stream)
        if rc:
            self._r = None
            raise BlswError("blsw_r1cs_create failed: %d" % rc)

    @classmethod
    def from_matrices(cls, mats, device=None):
        """a checker of a matrices() dict (any shape, e.g. one already built for the host check)"""
        return cls(device=device, _mats=mats)

    def close(self):
        if getattr(self, "_r", None):
            lib().blsw_r1cs_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _io(self, witness, instance, stream):
        """-> (n, instance pointer, instance stride, witness pointer, witness stride, stream) with the strides in field elements"""
        torch = self.torch

        def stride_of(t, need, what):
            assert t.is_cuda and t.device == self.device and t.dtype == torch.int64 and t.dim() == 3 and t.shape[2] == 6, what
            assert t.stride(2) == 1 and t.stride(1) == 6 and t.stride(0) % 6 == 0 and t.shape[1] >= need, "%s: [n, >= %d, 6] with rows of 6 contiguous limbs" % (what, need)
            return t.stride(0) // 6

        ws = stride_of(witness, self.n_witness, "witness")
        n = witness.shape[0]
        if instance is not None:
            ist = stride_of(instance, self.n_instance_vars, "instance")
            assert instance.shape[0] == n
        elif self.n_instance_vars > 1:
            raise BlswError("this circuit has %d public inputs: pass instance=" % (self.n_instance_vars - 1))
        else:
            ist = 0
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if s != torch.cuda.current_stream(self.device):
            self.buffer.record_stream(s)
        return n, instance.data_ptr() if instance is not None else None, ist, witness.data_ptr(), ws, s

    def _check(self, witness, instance, form, stream, want_unreduced):
        n, ip, ist, wp, ws, s = self._io(witness, instance, stream)
        with self.torch.cuda.stream(s):
            bad = self.torch.empty(n, dtype=self.torch.int64, device=self.device)
            unr = self.torch.empty(n, dtype=self.torch.int64, device=self.device) if want_unreduced else None
        rc = lib().blsw_r1cs_check(self._r, ip, ist, wp, ws, n, form, bad.data_ptr(), unr.data_ptr() if unr is not None else None, s.cuda_stream)
        if rc:
            raise BlswError("blsw_r1cs_check failed: %d" % rc)
        return bad, unr

    def which_is_unsatisfied(self, witness, instance=None, form=0, stream=None):
        """int64 [n]: index of each instance's first unsatisfied constraint, -1 when it satisfies the system (asynchronous on `stream`)"""
        return self._check(witness, instance, form, stream, False)[0]

    def is_satisfied(self, witness, instance=None, form=0, stream=None):
        """bool [n]"""
        return self.which_is_unsatisfied(witness, instance, form, stream) < 0

    def first_unreduced(self, witness, instance=None, form=0, stream=None):
        """int64 [n]: each instance's first index k of z = [instance | witness] with z_k >= p, or -1"""
        return self._check(witness, instance, form, stream, True)[1]

    def evaluate(self, witness, instance=None, form=0, rows=None, stream=None):
        """(az, bz, cz), int64 [n, count, 6] each: <A_j, z>, <B_j, z>, <C_j, z> for j in [begin, begin + count), reduced, in the input's form.
        rows = (begin, count); default all rows."""
        begin, count = rows if rows is not None else (0, self.n_constraints)
        n, ip, ist, wp, ws, s = self._io(witness, instance, stream)
        with self.torch.cuda.stream(s):
            out = [self.torch.empty((n, count, 6), dtype=self.torch.int64, device=self.device) for _ in range(3)]
        rc = lib().blsw_r1cs_evaluate(self._r, ip, ist, wp, ws, n, form, begin, count, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), s.cuda_stream)
        if rc:
            raise BlswError("blsw_r1cs_evaluate failed: %d" % rc)
        return tuple(out)

    def head_rows(self, n_keys):
        """the number of leading constraints that read nothing but the constant one and the allocation witnesses of the first n_keys keys (elements
        [0, n_keys * 1942) of the witness vector): the rows check_keyset evaluates and skip_head_rows=True leaves out (blsw_r1cs_handle_head_rows)."""
        rows = ctypes.c_uint64(0)
        rc = lib().blsw_r1cs_handle_head_rows(self._r, n_keys * SEG_PK_ALLOC, ctypes.byref(rows))
        if rc:
            raise BlswError("blsw_r1cs_handle_head_rows failed: %d" % rc)
        return rows.value

    def check_keyset(self, keyset, stream=None):
        """the committee, once: (row, unreduced) of the head rows on z = [1 | keyset.table] — the first unsatisfied row or -1, and the index of z
        (n_instance_vars + k) of the first table element >= p or -1. The table in either element form. Synchronises `stream`."""
        torch = self.torch
        assert isinstance(keyset, KeySet) and keyset.device == self.device
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if s != torch.cuda.current_stream(self.device):
            self.buffer.record_stream(s)
            keyset.buffer.record_stream(s)
        with torch.cuda.stream(s):
            out = torch.empty(2, dtype=torch.int64, device=self.device)
        rc = lib().blsw_r1cs_check_keyset(self._r, keyset._ks, out[0:].data_ptr(), out[1:].data_ptr(), s.cuda_stream)
        if rc:
            raise BlswError("blsw_r1cs_check_keyset failed: %d" % rc)
        with torch.cuda.stream(s):
            row, unreduced = out.tolist()
        return row, unreduced

    def _io_compact(self, layout, compact, instance, stream, keyset=None):
        """-> (n, instance pointer, instance stride, stream) for a step's compact buffer (uint8 cuda tensor of layout.total bytes)"""
        torch = self.torch
        assert isinstance(layout, (blsw_compact_layout_t, blsw_compact_layout_multi_t))
        assert keyset is None or (isinstance(keyset, KeySet) and keyset.device == self.device)
        assert compact.is_cuda and compact.device == self.device and compact.is_contiguous() and compact.dtype.itemsize == 1 and compact.numel() >= layout.total
        n, ip, ist = int(layout.n), None, 0
        if instance is not None:
            assert instance.is_cuda and instance.device == self.device and instance.dtype == torch.int64 and instance.dim() == 3 and instance.shape[2] == 6
            assert instance.stride(2) == 1 and instance.stride(1) == 6 and instance.stride(0) % 6 == 0 and instance.shape[0] == n and instance.shape[1] >= self.n_instance_vars
            ip, ist = instance.data_ptr(), instance.stride(0) // 6
        elif self.n_instance_vars > 1:
            raise BlswError("this circuit has %d public inputs and the compact form carries witnesses only: pass instance=" % (self.n_instance_vars - 1))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if s != torch.cuda.current_stream(self.device):
            self.buffer.record_stream(s)
            if keyset is not None:
                keyset.buffer.record_stream(s)
        return n, ip, ist, s

    def pair_families(self, layout):
        """the pair families of this system under a blsw_compact_layout_multi_t: [(first_row, rows_per_pair)], the blocks the compact check of an
        N+1-pair step evaluates with one pair per lane (blsw_r1cs_handle_pair_families; computed once per layout, the first call synchronises)"""
        return _pair_families(lambda *a: lib().blsw_r1cs_handle_pair_families(self._r, *a), layout)

    def _check_compact(self, layout, compact, instance, stream, want_unreduced, keyset=None, skip_head_rows=False, _use_families=True):
        if isinstance(layout, blsw_compact_layout_multi_t):
            if keyset is not None or skip_head_rows:
                raise BlswError("keyset= / skip_head_rows belong to a shared-keys aggregate step, not to the N+1-pair product")
            n, ip, ist, s = self._io_compact(layout, compact, instance, stream)
            with self.torch.cuda.stream(s):
                bad = self.torch.empty(n, dtype=self.torch.int64, device=self.device)
                unr = self.torch.empty(n, dtype=self.torch.int64, device=self.device) if want_unreduced else None
            rc = lib().blsw_r1cs_check_compact_multi_ex(self._r, ctypes.byref(layout), compact.data_ptr(), ip, ist, 1 if _use_families else 0, bad.data_ptr(),
                                                        unr.data_ptr() if unr is not None else None, s.cuda_stream)
            if rc:
                raise BlswError("blsw_r1cs_check_compact_multi failed: %d" % rc)
            return bad, unr
        if keyset is None and skip_head_rows:
            raise BlswError("skip_head_rows needs keyset=: only a shared-keys step has head rows to skip")
        n, ip, ist, s = self._io_compact(layout, compact, instance, stream, keyset)
        with self.torch.cuda.stream(s):
            bad = self.torch.empty(n, dtype=self.torch.int64, device=self.device)
            unr = self.torch.empty(n, dtype=self.torch.int64, device=self.device) if want_unreduced else None
        up = unr.data_ptr() if unr is not None else None
        if keyset is not None:
            rc = lib().blsw_r1cs_check_compact_keyset(self._r, ctypes.byref(layout), compact.data_ptr(), keyset._ks, 1 if skip_head_rows else 0, ip, ist, bad.data_ptr(), up,
                                                      s.cuda_stream)
        else:
            rc = lib().blsw_r1cs_check_compact(self._r, ctypes.byref(layout), compact.data_ptr(), ip, ist, bad.data_ptr(), up, s.cuda_stream)
        if rc:
            raise BlswError("blsw_r1cs_check_compact%s failed: %d" % ("_keyset" if keyset is not None else "", rc))
        return bad, unr

    def which_is_unsatisfied_compact(self, layout, compact, instance=None, stream=None, keyset=None, skip_head_rows=False):
        """which_is_unsatisfied of the layout.n instances of a step read straight from its compact buffer (WitnessEngine.submit_compact /
        compact_layout()): no expand_compact, no 34 MB-per-instance tensor. Montgomery form; instance as in which_is_unsatisfied.
        keyset: the step's KeySet (a shared-keys engine's step: its buffer carries no key rows, the set's table is the head of every vector).
        skip_head_rows: leave out the rows that read the head alone (head_rows(keyset.n_keys) of them) — check_keyset vouches for those once per
        set; reported rows keep their numbers."""
        return self._check_compact(layout, compact, instance, stream, False, keyset, skip_head_rows)[0]

    def is_satisfied_compact(self, layout, compact, instance=None, stream=None, keyset=None, skip_head_rows=False):
        """bool [layout.n]"""
        return self.which_is_unsatisfied_compact(layout, compact, instance, stream, keyset, skip_head_rows) < 0

    def first_unreduced_compact(self, layout, compact, instance=None, stream=None, keyset=None, skip_head_rows=False):
        """int64 [layout.n]: first index of z = [instance | witness] >= p among the instance vector and the staged rows (a bit cannot be), or -1.
        With keyset=: the buffer's witness k is reported at n_instance_vars + head_len + k; the head itself is never covered (check_keyset)."""
        return self._check_compact(layout, compact, instance, stream, True, keyset, skip_head_rows)[1]

    def evaluate_compact(self, layout, compact, instance=None, rows=None, stream=None, keyset=None, skip_head_rows=False):
        """evaluate() with z read from a step's compact buffer: (az, bz, cz), int64 [layout.n, count, 6] each, Montgomery form. keyset: as in
        which_is_unsatisfied_compact; any row window, head rows included (skip_head_rows has nothing to skip here and must stay False)."""
        if skip_head_rows:
            raise BlswError("evaluate_compact evaluates the window it is given: skip_head_rows does not apply")
        if isinstance(layout, blsw_compact_layout_multi_t) and keyset is not None:
            raise BlswError("keyset= belongs to a shared-keys aggregate step, not to the N+1-pair product")
        begin, count = rows if rows is not None else (0, self.n_constraints)
        n, ip, ist, s = self._io_compact(layout, compact, instance, stream, keyset)
        with self.torch.cuda.stream(s):
            out = [self.torch.empty((n, count, 6), dtype=self.torch.int64, device=self.device) for _ in range(3)]
        outs = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), s.cuda_stream)
        if isinstance(layout, blsw_compact_layout_multi_t):
            rc = lib().blsw_r1cs_evaluate_compact_multi(self._r, ctypes.byref(layout), compact.data_ptr(), ip, ist, begin, count, *outs)
        elif keyset is not None:
            rc = lib().blsw_r1cs_evaluate_compact_keyset(self._r, ctypes.byref(layout), compact.data_ptr(), keyset._ks, ip, ist, begin, count, *outs)
        else:
            rc = lib().blsw_r1cs_evaluate_compact(self._r, ctypes.byref(layout), compact.data_ptr(), ip, ist, begin, count, *outs)
        if rc:
            raise BlswError("blsw_r1cs_evaluate_compact%s failed: %d" % ("_keyset" if keyset is not None else "", rc))
        return tuple(out)


def layout_multi(msg_len, n_pairs, multi_inputs=0):
    """Segment table of the N+1-pair product; multi_inputs: mask of MULTI_*_INPUT (blsw_layout_multi_inputs), 0 = every argument Witness"""
    L = blsw_layout_t()
    if multi_inputs:
        rc = lib().blsw_layout_multi_inputs(msg_len, n_pairs, multi_inputs, ctypes.byref(L))
    else:
        rc = lib().blsw_layout_multi(msg_len, n_pairs, ctypes.byref(L))
    if rc:
        raise BlswError("blsw_layout_multi failed: %d" % rc)
    return {n: getattr(L, n) for n in _LAYOUT_FIELDS}


def verify_multi(parameters, public_keys, messages, signature, want_witness=True):
    """N+1-pair product of pairings: one signature over K (pk_j, msg_j) pairs per instance, i.e. constraints.rs:90-128 with
    product_of_pairings over slices of K + 1 prepared points. public_keys.xy [n, K, 12] int64, messages [n, K, msg_len] uint8,
    signature.xy [n, 24]. Returns (result int32 [n], witness [n, n_witness, 6] int64 or None).
    messages may be a UInt8 vector. With an argument allocated as Input (PublicKeyVar.new_input, UInt8.new_input_vec, SignatureVar.new_input; K >= 2)
    the circuit is the one of layout_multi(msg_len, K, mask): a one-step engine runs it and the call returns (result, witness, instance) with
    instance [n, n_instance_vars, 6] = every instance's instance_assignment."""
    torch = _require_cuda()
    assert isinstance(parameters, ParametersVar)
    msg_var = messages if isinstance(messages, UInt8) else UInt8(messages)
    mask = ((MULTI_KEYS_INPUT if public_keys.mode == "Input" else 0) | (MULTI_MSG_INPUT if msg_var.mode == "Input" else 0) |
            (MULTI_SIG_INPUT if signature.mode == "Input" else 0))
    pks, sig, messages = public_keys.xy.contiguous(), signature.xy.contiguous(), msg_var.bytes.contiguous()
    n, K = pks.shape[0], pks.shape[1]
    assert K >= 1 and messages.shape[:2] == (n, K) and sig.shape == (n, 24) and pks.shape == (n, K, 12)
    msg_len = messages.shape[2]
    if mask:
        if parameters.mode != "Constant":
            raise BlswError("verify_multi with Input arguments: ParametersVar allocated as %s is not offered (Constant)" % parameters.mode)
        if K < 2:
            raise BlswError("verify_multi with Input arguments needs at least two pairs (one pair: BlsSignatureVerifyGadget with pk_mode / sig_mode / msg_mode)")
        lay = layout_multi(msg_len, K, mask)
        # an N+1-pair engine is a staged one: one step per group, two group buffers
        eng = WitnessEngine(n, msg_len, max_steps=1, n_buffers=2, device=pks.device, reserve_bytes=n * lay["n_witness"] * 48 if want_witness else 0, n_pairs=K,
                            multi_inputs=mask)
        try:
            res = torch.empty(n, dtype=torch.int32, device=pks.device)
            wit = eng.new_witness_tensor() if want_witness else None
            inst = eng.new_instance_tensor()
            eng.submit_multi(pks, messages, sig, witness=wit, result=res, instance=inst)
            eng.flush()
            torch.cuda.synchronize(pks.device)
        finally:
            eng.close()
        return res, wit, inst
    lay = layout_multi(msg_len, K)
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_verify_multi_workspace_bytes(n, msg_len, K, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_verify_multi_workspace_bytes failed: %d" % rc)
    dev = pks.device
    check_capacity(dev, "verify_multi (n = %d, %d pairs)" % (n, K), wb.value, n * lay["n_witness"] * 48 if want_witness else 0)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty(n, dtype=torch.int32, device=dev)
    wit = torch.empty((n, lay["n_witness"], 6), dtype=torch.int64, device=dev) if want_witness else None
    rc = lib().blsw_verify_multi_batch(pks.data_ptr(), messages.data_ptr() if msg_len else None, msg_len, K, sig.data_ptr(), n, wit.data_ptr() if wit is not None else None,
                                       lay["n_witness"], res.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_verify_multi_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return res, wit


DIGEST_KEY, DIGEST_A = 0x9E3779B1, 0x85EBCA6B  # include/blsw.h: blsw_witness_digest


def witness_digest(witness, n_witness=None, out=None, stream=None):
    """blsw_witness_digest: [n, stride, 6] int64 cuda tensor -> [n, 2] int64 (two u64 sums, see include/blsw.h)."""
    torch = _require_cuda()
    assert witness.is_cuda and witness.is_contiguous() and witness.dim() == 3 and witness.shape[2] == 6
    n, stride = witness.shape[0], witness.shape[1]
    if out is None:
        out = torch.empty((n, 2), dtype=torch.int64, device=witness.device)
    s = stream if stream is not None else torch.cuda.current_stream(witness.device)
    rc = lib().blsw_witness_digest(witness.data_ptr(), stride, n, n_witness if n_witness is not None else stride, out.data_ptr(), s.cuda_stream)
    if rc:
        raise BlswError("blsw_witness_digest failed: %d" % rc)
    return out


def witness_digest_reference(words):
    """The same digest in numpy (host-side definition used by consumers / tests; include/blsw.h): `words` = the instance's u64 words."""
    import numpy as np

    x = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1).view(np.uint32).reshape(-1, 4)  # 16-byte pieces of little-endian u32 words
    key = ((np.arange(1, x.shape[0] + 1, dtype=np.uint64) * np.uint64(DIGEST_KEY)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    a = np.uint32(DIGEST_A)
    with np.errstate(over="ignore"):
        t = [(x[:, 0] + key), (x[:, 1] + key + a), (x[:, 2] + key + np.uint32(2) * a), (x[:, 3] + key + np.uint32(3) * a)]
        prod = t[0].astype(np.uint64) * t[1].astype(np.uint64) + t[2].astype(np.uint64) * t[3].astype(np.uint64)
        d0 = int(prod.sum(dtype=np.uint64))
        lo = int(((x[:, 0] ^ key) + (x[:, 2] ^ ~key)).sum(dtype=np.uint32))
        hi = int(((x[:, 1] ^ key) + (x[:, 3] ^ ~key)).sum(dtype=np.uint32))
    return [d0, lo | (hi << 32)]


def microbench(which, iters=4096, blocks=4096):
    """Measured device rates for the VALU roofline: which=0 v_mad_u64_u32/s, which=1 Fp products/s."""
    _require_cuda()
    v = ctypes.c_double(0)
    rc = lib().blsw_microbench(which, iters, blocks, ctypes.byref(v))
    if rc:
        raise BlswError("blsw_microbench failed: %d" % rc)
    return v.value


def fill_rate(tensor, reps=2):
    """blsw_fill_rate: bytes/s of a plain fill of `tensor` (a cuda tensor; overwritten) in the expansion's store geometry — the same-box HBM yardstick."""
    _require_cuda()
    v = ctypes.c_double(0)
    rc = lib().blsw_fill_rate(ctypes.c_void_p(tensor.data_ptr()), ctypes.c_uint64(tensor.numel() * tensor.element_size()), reps, ctypes.byref(v))
    if rc:
        raise BlswError("blsw_fill_rate failed: %d" % rc)
    return v.value


def hash_to_g2_batch(message, out=None, dst=None):
    """Batched hash_to_g2_with_cons values (hasher.rs:727-740): message [n, msg_len] uint8 cuda tensor -> [n, 24] int64 affine."""
    torch = _require_cuda()
    n, msg_len = message.shape
    wb = ctypes.c_uint64(0)
    lib().blsw_hash_to_g2_workspace_bytes(n, msg_len, ctypes.byref(wb))
    ws = torch.empty(wb.value, dtype=torch.uint8, device=message.device)
    if out is None:
        out = torch.empty((n, 24), dtype=torch.int64, device=message.device)
    rc = _dst_entry("blsw_hash_to_g2_batch", dst)(message.data_ptr(), msg_len, n, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(message.device).cuda_stream)
    if rc:
        raise BlswError("blsw_hash_to_g2_batch failed: %d" % rc)
    return out


ST_INVALID_SECRET_KEY = 5


def sign_batch(sk32_le, message, want_bytes=True, dst=None):
    """BLS::sign + PublicKey::from(&sk) for a batch (bls.rs:411-425, 183-195): sk32_le [n, 32] uint8 (little-endian Fr, as
    PrivateKey::try_from takes it), message [n, msg_len] uint8, cuda tensors.
    Returns dict(sig96, pk48 (uint8, None unless want_bytes), sig_xy [n,24], pk_xy [n,12] int64 Montgomery, status [n] int32)."""
    torch = _require_cuda()
    n, msg_len = message.shape
    assert sk32_le.shape == (n, 32) and sk32_le.is_contiguous() and message.is_contiguous()
    dev = message.device
    wb = ctypes.c_uint64(0)
    lib().blsw_hash_to_g2_workspace_bytes(n, msg_len, ctypes.byref(wb))
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    sig96 = torch.empty((n, 96), dtype=torch.uint8, device=dev) if want_bytes else None
    pk48 = torch.empty((n, 48), dtype=torch.uint8, device=dev) if want_bytes else None
    sig_xy = torch.empty((n, 24), dtype=torch.int64, device=dev)
    pk_xy = torch.empty((n, 12), dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    rc = _dst_entry("blsw_sign_batch", dst)(sk32_le.data_ptr(), message.data_ptr(), msg_len, n, sig96.data_ptr() if want_bytes else None, sig_xy.data_ptr(),
                               pk48.data_ptr() if want_bytes else None, pk_xy.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_sign_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return {"sig96": sig96, "pk48": pk48, "sig_xy": sig_xy, "pk_xy": pk_xy, "status": status}


def hash_to_field_batch(message, dst=None):
    """hash_to_field of RFC 9380 for G2 on its own (blsw_hash_to_field_batch): message [n, msg_len] uint8 cuda tensor -> [n, 4, 6] int64 Montgomery
    (u0.c0, u0.c1, u1.c0, u1.c1) under the tag dst (None = DST_DEFAULT). No workspace."""
    torch = _require_cuda()
    n, msg_len = message.shape
    assert message.dtype == torch.uint8 and message.is_contiguous()
    out = torch.empty((n, 4, 6), dtype=torch.int64, device=message.device)
    t = _dst_struct(dst) if dst is not None else None
    rc = lib().blsw_hash_to_field_batch(message.data_ptr() if msg_len else None, msg_len, n, ctypes.byref(t) if t is not None else None, out.data_ptr(),
                                        torch.cuda.current_stream(message.device).cuda_stream)
    if rc:
        raise BlswError("blsw_hash_to_field_batch failed: %d" % rc)
    return out


def pop_prove(sk32_le):
    """PopProve of the signature draft's POP ciphersuite for a batch (blsw_pop_prove_batch): sk32_le [n, 32] uint8 cuda tensor (little-endian Fr) ->
    dict(pk48 [n, 48], proof96 [n, 96] uint8, status [n] int32 as sign_batch's): proof = sk * hash_to_g2(pk48, DST_POP)."""
    torch = _require_cuda()
    n = sk32_le.shape[0]
    assert sk32_le.shape == (n, 32) and sk32_le.dtype == torch.uint8 and sk32_le.is_contiguous()
    dev = sk32_le.device
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_hash_to_g2_workspace_bytes(n, 48, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_hash_to_g2_workspace_bytes failed: %d" % rc)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    proof96 = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    pk48 = torch.empty((n, 48), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    rc = lib().blsw_pop_prove_batch(sk32_le.data_ptr(), n, proof96.data_ptr(), pk48.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_pop_prove_batch failed: %d" % rc)
    torch.cuda.synchronize(dev)
    return {"pk48": pk48, "proof96": proof96, "status": status}


def pop_verify(pk48, proof96, want_status=False):
    """PopVerify for a batch (blsw_pop_verify_batch): uint8 cuda tensors pk48 [n, 48], proof96 [n, 96] -> int32 [n] verdicts — verify_batch with the
    key's own bytes as the message under DST_POP, KeyValidate included —, optionally with the decode statuses [n, 2] (key, proof)."""
    torch = _require_cuda()
    n = pk48.shape[0]
    assert pk48.shape == (n, 48) and proof96.shape == (n, 96) and pk48.is_contiguous() and proof96.is_contiguous()
    dev = pk48.device
    wb = ctypes.c_uint64(0)
    rc = lib().blsw_verify_workspace_bytes(n, 48, ctypes.byref(wb))
    if rc:
        raise BlswError("blsw_verify_workspace_bytes failed: %d" % rc)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    rc = lib().blsw_pop_verify_batch(pk48.data_ptr(), proof96.data_ptr(), n, res.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise BlswError("blsw_pop_verify_batch failed: %d" % rc)
    return (res, status) if want_status else res
