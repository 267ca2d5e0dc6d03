"""ctypes binding of the C-ABI in ``include/preganplus.h``.

This is the binding a maintainer of the reference would add:
the reference's interface for this path is Python, so the FFI is ctypes.
There is no fallback: if the HIP library is missing, importing the product
path raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PGP_LIB", os.path.join(_HERE, "_lib", "libpreganplus.so"))

PGP_OK = 0
_ERRS = {-1: "PGP_ERR_ARG", -2: "PGP_ERR_UNSUPPORTED", -3: "PGP_ERR_HIP", -4: "PGP_ERR_STATE"}

_lib = None

# A/B switches removed in round 5: the library and the
# Python host read none of them any more.  Setting one warns instead of
# silently measuring the default; PGP_INIT_SEED became the recoveries'
# ``init_seed`` argument.
REMOVED_ENV = ("PGP_TUNE_SIDE_STREAM", "PGP_TUNE_SIDE_MIN_TOKENS", "PGP_TUNE_DEC_DWS", "PGP_TUNE_SIDE_EARLY",
               "PGP_TUNE_EARLY_FLUSH", "PGP_TF_SPREAD", "PGP_C3_GAN_LATE", "PGP_INIT_SEED", "PGP_SAVE_GAN_INTERVAL")


def _warn_removed_env():
    import warnings
    for k in REMOVED_ENV:
        if k in os.environ:
            hint = " (use the init_seed argument)" if k == "PGP_INIT_SEED" else ""
            warnings.warn(f"{k} is no longer read by preganplus_amd{hint}; it has no effect", RuntimeWarning,
                          stacklevel=3)


class NativeError(RuntimeError):
    pass


i32, i64, sz, f32, f64 = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_float, ctypes.c_double
vp = stream = ctypes.c_void_p  # device pointers and handles; `stream` marks a prototype's hipStream_t


# ctypes mirrors of the header's structs and callback: pgp_adam_tensor, pgp_online_tensor, pgp_online_desc
class _AdamTensor(ctypes.Structure):
    _fields_ = [("offset", i64), ("n", i32), ("active", i32), ("step_size", f32), ("bc2_sqrt", f32)]


class _OnlineTensor(ctypes.Structure):
    _fields_ = [("offset", i64), ("n", i32), ("section", i32), ("cond", i32), ("step", f64)]


class _OnlineDesc(ctypes.Structure):
    _fields_ = ([(n, i32) for n in ("n_hosts", "n_env", "n_rows", "n_protos")]
                + [(n, vp) for n in ("series", "train_max", "sched", "envs", "P", "G", "exp_avg", "exp_avg_sq",
                                     "tune_ws", "logits", "protos", "windows", "y", "cls", "state", "mult", "tgt",
                                     "loss", "inc", "dp_ws", "adam_rows", "cond_steps", "gan_ws", "ns", "probs",
                                     "emb", "sim_out", "target")]
                + [("tensors", ctypes.POINTER(_OnlineTensor)), ("n_tensors", i32), ("n_cond", i32), ("lr", f64 * 3)]
                + [(n, f64) for n in ("weight_decay", "beta1", "beta2", "eps", "update_min", "decay")])


_COLL_FN = ctypes.CFUNCTYPE(i32, vp, i32, vp)  # pgp_collective_fn(user, which, stream)

# Every entry point of include/preganplus.h, in the header's order: name -> (restype, argtypes); ctypes would pass
# ints as 32-bit C ints and truncate device pointers without them.  tests/test_abi_table.py holds it to the header.
cstr, pi32, pf64, pvp = ctypes.c_char_p, ctypes.POINTER(i32), ctypes.POINTER(f64), ctypes.POINTER(vp)
adam = ctypes.POINTER(_AdamTensor)
SIGNATURES = {
    "pgp_abi_version": (i32, []),
    "pgp_last_error": (cstr, []),
    "pgp_supported_hosts": (i32, [pi32, i32]),
    "pgp_create": (i32, [i32, i32, pvp]),
    "pgp_destroy": (i32, [vp]),
    "pgp_weight_blob_len": (sz, [i32, i32]),
    "pgp_load_weights": (i32, [vp, pf64, sz]),
    "pgp_reserve": (i32, [vp, i32]),
    "pgp_forward": (i32, [vp, i32] + [vp] * 11 + [stream]),
    "pgp_forward_stage": (i32, [vp, i32, i32] + [vp] * 11 + [stream]),
    "pgp_migrations": (i32, [i32, i32] + [vp] * 5 + [stream]),
    "pgp_embedding": (i32, [i32, i32] + [vp] * 3 + [stream]),
    "pgp_decoder_split": (i32, [vp, i32]),
    "pgp_encoder_split": (i32, [vp, i32]),
    "pgp_encoder_form_info": (i32, [i32] + [pi32] * 4),
    "pgp_gan_split": (i32, [vp, i32]),
    "pgp_schedule_onehot": (i32, [i32, i32, vp, vp, stream]),
    "pgp_create_fpe": (i32, [i32, pvp]),
    "pgp_fpe_weight_blob_len": (sz, [i32]),
    "pgp_forward_fpe": (i32, [vp, i32] + [vp] * 11 + [stream]),
    "pgp_forward_fpe_stage": (i32, [vp, i32, i32] + [vp] * 11 + [stream]),
    "pgp_master_len": (sz, [i32]),
    "pgp_tune_workspace_len": (sz, [i32, i32]),
    "pgp_gan_workspace_len": (sz, [i32, i32]),
    "pgp_master_offset": (sz, [i32, i32]),
    "pgp_tune_forward": (i32, [i32, i32] + [vp] * 6 + [stream]),
    "pgp_tune_backward": (i32, [i32, i32] + [vp] * 8 + [stream]),
    "pgp_tune_backward_prefix": (i32, [i32, i32, i32] + [vp] * 8 + [stream]),
    "pgp_tune_set_side_stream": (i32, [stream]),
    "pgp_tune_reserve_cus": (i32, [i32]),
    "pgp_tune_timing": (i32, [i32]),
    "pgp_tune_fused_ms": (i32, [vp]),
    "pgp_tune_plan_info": (i32, [i32, i32, i32, pi32, i32]),
    "pgp_gan_plan_info": (i32, [i32, i32]),
    "pgp_tune_targets": (i32, [i32, i32] + [vp] * 5 + [f64, f64] + [vp] * 3 + [stream]),
    "pgp_tune_step1": (i32, [i32, i32] + [vp] * 6 + [f64, f64] + [vp] * 3 + [stream]),
    "pgp_tune_dropout_mask_len": (sz, [i32]),
    "pgp_tune_step1_dropout": (i32, [i32, i32] + [vp] * 6 + [f64, f64] + [vp] * 3 + [f32, vp, i32, stream]),
    "pgp_tune_dropout_masks": (i32, [i32, f32, vp, i32, vp, stream]),
    "pgp_tune_forward_many": (i32, [i32, i32] + [vp] * 4 + [stream]),
    "pgp_forward1": (i32, [i32, i32] + [vp] * 12 + [stream]),
    "pgp_tune_step1_many": (i32, [i32] * 5 + [vp] * 7 + [f64, f64] + [vp] * 3 + [f32, vp, stream]),
    "pgp_tune_forward_cells": (i32, [i32] * 3 + [vp] * 5 + [stream]),
    "pgp_tune_scores_many": (i32, [i32] * 4 + [vp] * 8 + [stream]),
    "pgp_forward1_many": (i32, [i32] * 3 + [vp] * 13 + [stream]),
    "pgp_tune_dataset": (i32, [i32] * 3 + [vp] * 6 + [stream]),
    "pgp_tune_dataset_cells": (i32, [i32] * 3 + [vp] * 8 + [stream]),
    "pgp_tune_targets_dp_workspace_len": (sz, [i32]),
    "pgp_tune_targets_dp": (i32, [i32] * 3 + [vp] * 5 + [f64] + [vp] * 5 + [stream]),
    "pgp_tune_state_apply": (i32, [i32, vp, vp, f64, i32, pi32, vp, vp, f64, f64, f64, stream]),
    "pgp_gan_forward": (i32, [i32, i32] + [vp] * 6 + [stream]),
    "pgp_gan_disc_backward": (i32, [i32, i32] + [vp] * 4 + [stream]),
    "pgp_gan_gen_backward": (i32, [i32, i32] + [vp] * 3 + [stream]),
    "pgp_gan_probs": (i32, [i32, i32, vp, vp, stream]),
    "pgp_adamw": (i32, [vp] * 4 + [f32] * 5 + [adam, i32, stream]),
    "pgp_adamw_table": (i32, [vp] * 4 + [f32] * 5 + [adam, i32, vp, stream]),
    "pgp_adamw_table_many": (i32, [i32, i64, vp] + [vp] * 4 + [f32] * 5 + [adam, i32, vp, i64, stream]),
    "pgp_gan_forward1": (i32, [i32] + [vp] * 6 + [stream]),
    "pgp_gan_step1": (i32, [i32] + [vp] * 5 + [f32] * 6 + [adam, i32, vp] + [adam, i32, vp] + [vp] * 3 + [stream]),
    "pgp_gan_forward1_many": (i32, [i32, i32] + [vp] * 7 + [stream]),
    "pgp_gan_step1_many": (i32, [i32, i32] + [vp] * 6 + [f32] * 6 + [adam, i32, vp, i64] + [adam, i32, vp, i64]
                           + [vp] * 3 + [stream]),
    # the same five with beta1 / beta2 as doubles (1 - beta rounded once, torch's moment weights): what this package calls
    "pgp_adamw_d": (i32, [vp] * 4 + [f32, f32, f64, f64, f32] + [adam, i32, stream]),
    "pgp_adamw_table_d": (i32, [vp] * 4 + [f32, f32, f64, f64, f32] + [adam, i32, vp, stream]),
    "pgp_adamw_table_many_d": (i32, [i32, i64, vp] + [vp] * 4 + [f32, f32, f64, f64, f32]
                               + [adam, i32, vp, i64, stream]),
    "pgp_gan_step1_d": (i32, [i32] + [vp] * 5 + [f32, f32, f32, f64, f64, f32] + [adam, i32, vp] + [adam, i32, vp]
                        + [vp] * 3 + [stream]),
    "pgp_gan_step1_many_d": (i32, [i32, i32] + [vp] * 6 + [f32, f32, f32, f64, f64, f32] + [adam, i32, vp, i64]
                             + [adam, i32, vp, i64] + [vp] * 3 + [stream]),
    "pgp_online_create": (i32, [ctypes.POINTER(_OnlineDesc), pvp]),
    "pgp_online_destroy": (i32, [vp]),
    "pgp_online_step": (i32, [vp, stream, stream, _COLL_FN, vp]),
    "pgp_online_timing": (i32, [vp, i32]),
    "pgp_online_issue_worker": (i32, [vp, i32]),
    "pgp_online_stage_ms": (i32, [vp, vp]),
    "pgp_online_steps": (i32, [vp, vp, i32]),
    "pgp_online_gan_step": (i32, [vp, stream]),
    "pgp_fpe_param_len": (sz, [i32]),
    "pgp_fpe_train_step": (i32, [i32, i32] + [vp] * 7 + [f64, f64, vp, stream]),
    "pgp_fpe_forward_many": (i32, [i32, i32] + [vp] * 5 + [stream]),
    "pgp_fpe_train_steps": (i32, [i32] * 3 + [vp] * 9 + [f64, f64, f32, f32, f64, f64, f32] + [adam, i32, vp, vp, stream]),
    "pgp_fpe_train_steps_many": (i32, [i32] * 3 + [vp, i64] + [vp] * 3 + [i64] + [vp] * 8
                                 + [f64, f64, f32, f32, f64, f64, f32] + [adam, i32, vp, stream]),
    "pgp_fpe_forward_many_cells": (i32, [i32, i32, vp, i64, vp, i64] + [vp] * 5 + [stream]),
    "pgp_fpe_forward1": (i32, [i32, i32] + [vp] * 14 + [stream]),
    "pgp_fpe_forward1_many": (i32, [i32] * 3 + [vp] * 7 + [i64] + [vp] * 8 + [stream]),
    "pgp_load_weights_master": (i32, [vp, vp, pf64]),
    "pgp_repack_master": (i32, [vp, vp, vp, stream]),
    "pgp_repack_master_sections": (i32, [vp, vp, vp, i32, stream]),
    "pgp_gobi_weight_len": (sz, [i32]),
    "pgp_gobi_create": (i32, [i32, vp, sz, pvp]),
    "pgp_gobi_destroy": (i32, [vp]),
    "pgp_gobi_last_error": (cstr, []),
    "pgp_gobi_optimize": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, stream]),
    "pgp_gobi_train_steps": (i32, [i32] * 3 + [vp] * 6 + [i64] + [f64] * 5 + [vp, stream]),
    "pgp_gobi_train_eval": (i32, [i32] * 3 + [vp] * 5 + [stream]),
    "pgp_gobi_train_steps_many": (i32, [i32, i32, vp, i64, vp, vp, i64] + [vp] * 6 + [stream]),
    "pgp_gobi_train_eval_many": (i32, [i32, i32, vp, i64, vp, vp, i64] + [vp] * 4 + [stream]),
    "pgp_gobi_create_many": (i32, [i32, i32, vp, sz, pvp]),
    "pgp_gobi_model_count": (i32, [vp]),
    "pgp_gobi_set_model": (i32, [vp, i32, vp, sz]),
    "pgp_gobi_optimize_groups": (i32, [vp, i32, i32] + [vp] * 5 + [i32, vp, stream]),
    "pgp_gobi_plan_groups": (i32, [i32, vp, i32, vp, i32]),
    "pgp_gobi_so_optimize": (i32, [vp, i32] + [vp] * 4 + [i32, vp, i32, vp, vp, stream]),
    "pgp_gobi_so_optimize_groups": (i32, [vp, i32, i32] + [vp] * 5 + [i32, vp, i32, vp, vp, stream]),
    "pgp_sim_env_len": (sz, [i32]),
    "pgp_simulate": (i32, [i32, i32] + [vp] * 5 + [stream]),
}
del i32, i64, sz, f32, f64, vp, stream, cstr, pi32, pf64, pvp, adam


def bind(L):
    """Give every entry point that ``L`` exports its SIGNATURES types.  An entry an
    older build lacks (PGP_LIB, tools/ab_bench.py) is skipped and named in
    ``L._pgp_missing``; calling it raises ctypes' AttributeError as before."""
    if not hasattr(L, "_pgp_missing"):
        missing = []
        for name, (restype, argtypes) in SIGNATURES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.argtypes, fn.restype = argtypes, restype
            else:
                missing.append(name)
        L._pgp_missing = tuple(missing)
    return L


def lib():
    """Load libpreganplus.so (built by ``make`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    _warn_removed_env()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"HIP library not found at {LIB_PATH}; build it with `make` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc, what=""):
    if rc != PGP_OK:
        msg = lib().pgp_last_error().decode(errors="replace")
        raise NativeError(f"{what}: {_ERRS.get(rc, rc)}: {msg}")


def supported_hosts():
    buf = (ctypes.c_int * 16)()
    n = lib().pgp_supported_hosts(buf, 16)
    return [buf[i] for i in range(n)]
