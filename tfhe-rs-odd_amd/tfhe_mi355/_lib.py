"""ctypes binding of lib/libtfhe_mi355.so (the C ABI declared in include/tfhe_mi355.h).

The HIP engine is the product path: there is no CPU fallback.  If the shared library is
missing, loading fails loudly.  torch is imported first (when available) so that the engine
and torch share one HIP runtime (torch bundles libamdhip64.so with the same SONAME).
"""
from __future__ import annotations

import ctypes
import os

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("TFHE_MI355_LIB") or os.path.join(_PKG_ROOT, "lib", "libtfhe_mi355.so")

u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
vp = ctypes.c_void_p
sz = ctypes.c_size_t


class TfheMi355Parameters(ctypes.Structure):
    _fields_ = [
        ("lwe_dimension", ctypes.c_uint32),
        ("glwe_dimension", ctypes.c_uint32),
        ("polynomial_size", ctypes.c_uint32),
        ("pbs_base_log", ctypes.c_uint32),
        ("pbs_level", ctypes.c_uint32),
        ("ks_base_log", ctypes.c_uint32),
        ("ks_level", ctypes.c_uint32),
        ("message_modulus", ctypes.c_uint32),
        ("carry_modulus", ctypes.c_uint32),
        ("grouping_factor", ctypes.c_uint32),
    ]


class TfheMi355ServerKeyInfo(ctypes.Structure):
    _fields_ = [
        ("params", TfheMi355Parameters),
        ("pbs_order", ctypes.c_uint32),
        ("deterministic_execution", ctypes.c_uint32),
        ("max_degree", ctypes.c_uint64),
        ("max_noise_level", ctypes.c_uint64),
        ("ksk_seed_lo", ctypes.c_uint64),
        ("ksk_seed_hi", ctypes.c_uint64),
        ("bsk_seed_lo", ctypes.c_uint64),
        ("bsk_seed_hi", ctypes.c_uint64),
    ]


class TfheMi355LweSource(ctypes.Structure):
    """kind: 0 expanded rows, 1 compact list, 2 seeded list (one seed), 3 seeded rows (a seed each); data and
    seeds are host pointers for the host-pointer calls, device pointers for the _async calls."""
    _fields_ = [
        ("kind", ctypes.c_uint32),
        ("lwe_dimension", ctypes.c_uint32),
        ("data", ctypes.c_void_p),
        ("seeds", ctypes.c_void_p),
    ]


BLOCK_OP_TERMS = 4


class TfheMi355BlockOpTerm(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("stride", ctypes.c_uint64), ("scalar", ctypes.c_uint64)]


class TfheMi355BlockOp(ctypes.Structure):
    """dst rows = sum of scalar * src rows + body_add on the last word (device pointers, strides in words;
    src NULL: term absent)."""
    _fields_ = [
        ("dst", ctypes.c_void_p),
        ("dst_stride", ctypes.c_uint64),
        ("body_add", ctypes.c_uint64),
        ("term", TfheMi355BlockOpTerm * BLOCK_OP_TERMS),
    ]


class TfheMi355ClearBlockOp(ctypes.Structure):
    """A block op with a clear digit per row: digit(r) = ((negate ? -d_clear[r] : d_clear[r]) >> clear_shift) &
    (2^clear_bits - 1); digit * clear_scale goes on the body of row r, lut_base + digit into d_lut_index[r]."""
    _fields_ = [
        ("op", TfheMi355BlockOp),
        ("d_clear", ctypes.c_void_p),
        ("clear_scale", ctypes.c_uint64),
        ("d_lut_index", ctypes.c_void_p),
        ("clear_negate", ctypes.c_uint32),
        ("clear_shift", ctypes.c_uint32),
        ("clear_bits", ctypes.c_uint32),
        ("lut_base", ctypes.c_uint32),
    ]


class TfheMi355CiphertextInfo(ctypes.Structure):
    _fields_ = [
        ("lwe_dimension", ctypes.c_uint32),
        ("pbs_order", ctypes.c_uint32),
        ("count", ctypes.c_uint64),
        ("degree", ctypes.c_uint64),
        ("message_modulus", ctypes.c_uint64),
        ("carry_modulus", ctypes.c_uint64),
        ("noise_level", ctypes.c_uint64),
        ("data_offset", ctypes.c_uint64),
        ("data_words", ctypes.c_uint64),
        ("seed_lo", ctypes.c_uint64),
        ("seed_hi", ctypes.c_uint64),
    ]


u8p = ctypes.POINTER(ctypes.c_uint8)

# (name, restype, argtypes) -- every symbol declared in include/tfhe_mi355.h
SIGNATURES = [
    ("tfhe_mi355_last_error", ctypes.c_char_p, []),
    ("tfhe_mi355_device_count", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("tfhe_mi355_host_alloc", ctypes.c_int, [sz, ctypes.POINTER(vp)]),
    ("tfhe_mi355_host_free", ctypes.c_int, [vp]),
    ("tfhe_mi355_context_create", ctypes.c_int,
     [ctypes.POINTER(TfheMi355Parameters), ctypes.c_int, ctypes.POINTER(vp)]),
    ("tfhe_mi355_context_create_devices", ctypes.c_int,
     [ctypes.POINTER(TfheMi355Parameters), ctypes.POINTER(ctypes.c_int), sz, ctypes.POINTER(vp)]),
    ("tfhe_mi355_context_devices", ctypes.c_int, [vp, ctypes.POINTER(sz)]),
    ("tfhe_mi355_context_replication", ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_char_p)]),
    ("tfhe_mi355_context_device_context", ctypes.c_int, [vp, sz, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int)]),
    ("tfhe_mi355_context_destroy", ctypes.c_int, [vp]),
    ("tfhe_mi355_bootstrap_key_upload", ctypes.c_int, [vp, u64p, sz]),
    ("tfhe_mi355_bootstrap_key_convert_async", ctypes.c_int, [vp, vp, sz, vp]),
    ("tfhe_mi355_bootstrap_key_fourier", ctypes.c_int, [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]),
    ("tfhe_mi355_bootstrap_key_fourier_set_ready", ctypes.c_int, [vp]),
    ("tfhe_mi355_keyswitch_key_upload", ctypes.c_int, [vp, u64p, sz]),
    ("tfhe_mi355_keyswitch_key_upload_async", ctypes.c_int, [vp, vp, sz, vp]),
    ("tfhe_mi355_keyswitch_key_device", ctypes.c_int, [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]),
    ("tfhe_mi355_keyswitch_key_set_ready", ctypes.c_int, [vp]),
    ("tfhe_mi355_programmable_bootstrap", ctypes.c_int, [vp, u64p, u64p, u64p, sz, u32p, sz]),
    ("tfhe_mi355_programmable_bootstrap_async", ctypes.c_int, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_programmable_bootstrap_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_keyswitch", ctypes.c_int, [vp, u64p, u64p, sz]),
    ("tfhe_mi355_keyswitch_async", ctypes.c_int, [vp, vp, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_keyswitch_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_lwe_keyswitch_key_create", ctypes.c_int,
     [vp, u64p, sz, sz, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp)]),
    ("tfhe_mi355_lwe_keyswitch_key_destroy", ctypes.c_int, [vp]),
    ("tfhe_mi355_keyswitch_with_key", ctypes.c_int, [vp, vp, u64p, u64p, sz]),
    ("tfhe_mi355_keyswitch_with_key_async", ctypes.c_int, [vp, vp, vp, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_keyswitch_with_key_scratch", ctypes.c_int, [vp, vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_keyswitch_programmable_bootstrap", ctypes.c_int, [vp, u64p, u64p, u64p, sz, u32p, sz]),
    ("tfhe_mi355_keyswitch_programmable_bootstrap_async", ctypes.c_int,
     [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_keyswitch_programmable_bootstrap_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_programmable_bootstrap_keyswitch", ctypes.c_int, [vp, u64p, u64p, u64p, sz, u32p, sz]),
    ("tfhe_mi355_programmable_bootstrap_keyswitch_async", ctypes.c_int,
     [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_programmable_bootstrap_keyswitch_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_fill_accumulator", ctypes.c_int, [ctypes.POINTER(TfheMi355Parameters), u64p, u64p]),
    ("tfhe_mi355_client_gen_binary_key", ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, u64p, sz]),
    ("tfhe_mi355_client_gen_bootstrap_key", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_double, u64p, ctypes.c_uint32]),
    ("tfhe_mi355_blind_rotate", ctypes.c_int, [vp, u64p, u64p, u64p, ctypes.c_size_t, u32p, ctypes.c_size_t]),
    ("tfhe_mi355_blind_rotate_async", ctypes.c_int,
     [vp, vp, vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]),
    ("tfhe_mi355_lwe_scalar_mul_add_async", ctypes.c_int,
     [vp, vp, vp, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp]),
    ("tfhe_mi355_lwe_block_layer_async", ctypes.c_int,
     [vp, ctypes.POINTER(TfheMi355BlockOp), ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp]),
    ("tfhe_mi355_lwe_clear_block_layer_async", ctypes.c_int,
     [vp, ctypes.POINTER(TfheMi355ClearBlockOp), ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp]),
    ("tfhe_mi355_trivial_pbs_async", ctypes.c_int, [vp, vp, ctypes.c_size_t, ctypes.c_size_t, vp, vp]),
    ("tfhe_mi355_client_gen_multi_bit_bootstrap_key", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, u64p, ctypes.c_uint32]),
    ("tfhe_mi355_client_gen_keyswitch_key", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_double, u64p]),
    ("tfhe_mi355_packing_keyswitch_key_upload", ctypes.c_int, [vp, u64p, sz, ctypes.c_uint32, ctypes.c_uint32]),
    ("tfhe_mi355_packing_keyswitch", ctypes.c_int, [vp, u64p, u64p, sz]),
    ("tfhe_mi355_packing_keyswitch_async", ctypes.c_int, [vp, vp, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_packing_keyswitch_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_relinearization_key_upload", ctypes.c_int, [vp, u64p, sz, ctypes.c_uint32, ctypes.c_uint32]),
    ("tfhe_mi355_glwe_mult", ctypes.c_int, [vp, u64p, u64p, ctypes.c_uint32, ctypes.c_int, u64p, sz]),
    ("tfhe_mi355_glwe_mult_async", ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_int, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_glwe_mult_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_lwe_mult", ctypes.c_int, [vp, u64p, u64p, ctypes.c_uint32, u64p, sz]),
    ("tfhe_mi355_lwe_mult_async", ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_lwe_mult_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_glwe_poly_mul", ctypes.c_int, [vp, u64p, sz, u64p, sz, sz, ctypes.c_int, u64p]),
    ("tfhe_mi355_glwe_poly_mul_async", ctypes.c_int, [vp, vp, sz, vp, sz, sz, ctypes.c_int, vp, vp]),
    ("tfhe_mi355_ggsw_external_product", ctypes.c_int,
     [vp, u64p, sz, ctypes.c_uint32, ctypes.c_uint32, u32p, u64p, u64p, sz]),
    ("tfhe_mi355_ggsw_external_product_async", ctypes.c_int,
     [vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, sz, vp]),
    ("tfhe_mi355_ggsw_cmux", ctypes.c_int,
     [vp, u64p, sz, ctypes.c_uint32, ctypes.c_uint32, u32p, u64p, u64p, u64p, sz]),
    ("tfhe_mi355_ggsw_cmux_async", ctypes.c_int,
     [vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, sz, vp]),
    ("tfhe_mi355_ggsw_list_fourier_bytes", ctypes.c_int, [vp, sz, ctypes.c_uint32, ctypes.POINTER(sz)]),
    ("tfhe_mi355_ggsw_list_convert_async", ctypes.c_int, [vp, vp, sz, ctypes.c_uint32, vp, vp]),
    ("tfhe_mi355_vertical_packing", ctypes.c_int,
     [vp, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p, sz, sz, u32p, sz, u64p]),
    ("tfhe_mi355_vertical_packing_async", ctypes.c_int,
     [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, sz, sz, vp, sz, vp, vp, sz, vp]),
    ("tfhe_mi355_vertical_packing_scratch", ctypes.c_int, [vp, sz, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_pfpksk_list_upload", ctypes.c_int, [vp, u64p, sz, ctypes.c_uint32, ctypes.c_uint32]),
    ("tfhe_mi355_private_functional_packing_keyswitch", ctypes.c_int, [vp, u64p, u64p, sz]),
    ("tfhe_mi355_private_functional_packing_keyswitch_async", ctypes.c_int, [vp, vp, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_private_functional_packing_keyswitch_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_extract_bits", ctypes.c_int, [vp, u64p, ctypes.c_uint32, ctypes.c_uint32, u64p, sz]),
    ("tfhe_mi355_extract_bits_async", ctypes.c_int,
     [vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_extract_bits_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_circuit_bootstrap", ctypes.c_int,
     [vp, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p, sz]),
    ("tfhe_mi355_circuit_bootstrap_async", ctypes.c_int,
     [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_circuit_bootstrap_scratch", ctypes.c_int, [vp, ctypes.c_uint32, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_circuit_bootstrap_vertical_packing", ctypes.c_int,
     [vp, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p, sz, sz, sz, u32p, sz, u64p]),
    ("tfhe_mi355_circuit_bootstrap_vertical_packing_async", ctypes.c_int,
     [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, sz, sz, sz, vp, sz, vp, vp, sz, vp]),
    ("tfhe_mi355_circuit_bootstrap_vertical_packing_scratch", ctypes.c_int,
     [vp, ctypes.c_uint32, ctypes.c_uint32, sz, sz, sz, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_client_gen_pfpksk_list", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_double, u64p, ctypes.c_uint32]),
    ("tfhe_mi355_client_gen_packing_keyswitch_key", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_double, u64p, ctypes.c_uint32]),
    ("tfhe_mi355_client_gen_relinearization_key", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double,
      u64p]),
    ("tfhe_mi355_bootstrap_key_upload_seeded", ctypes.c_int, [vp, u64p, sz, ctypes.c_uint64, ctypes.c_uint64]),
    ("tfhe_mi355_keyswitch_key_upload_seeded", ctypes.c_int, [vp, u64p, sz, ctypes.c_uint64, ctypes.c_uint64]),
    ("tfhe_mi355_csprng_mask_words", ctypes.c_int, [vp, ctypes.c_uint64, ctypes.c_uint64, u64p, sz]),
    # compressed ciphertext ingress
    ("tfhe_mi355_lwe_expand", ctypes.c_int, [vp, ctypes.POINTER(TfheMi355LweSource), sz, u64p]),
    ("tfhe_mi355_lwe_expand_scratch", ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_uint32, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_lwe_expand_async", ctypes.c_int, [vp, ctypes.POINTER(TfheMi355LweSource), sz, vp, vp, sz, vp]),
    ("tfhe_mi355_apply_from", ctypes.c_int,
     [vp, ctypes.c_int, ctypes.POINTER(TfheMi355LweSource), u64p, u64p, sz, u32p, sz]),
    ("tfhe_mi355_apply_from_scratch", ctypes.c_int, [vp, ctypes.c_int, ctypes.c_uint32, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_apply_from_async", ctypes.c_int,
     [vp, ctypes.c_int, ctypes.POINTER(TfheMi355LweSource), vp, vp, sz, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_compact_ciphertext_list_inspect", ctypes.c_int, [u8p, sz, ctypes.POINTER(TfheMi355CiphertextInfo)]),
    ("tfhe_mi355_compressed_ciphertext_inspect", ctypes.c_int, [u8p, sz, ctypes.POINTER(TfheMi355CiphertextInfo)]),
    ("tfhe_mi355_client_gen_compact_public_key", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, ctypes.c_double, u64p]),
    ("tfhe_mi355_client_compact_encrypt", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, sz, ctypes.c_double, ctypes.c_double, u64p]),
    ("tfhe_mi355_client_seeded_lwe_encrypt", ctypes.c_int,
     [ctypes.c_uint64, u64p, u64p, ctypes.c_uint32, u64p, sz, ctypes.c_double, u64p]),
    ("tfhe_mi355_client_seeded_lwe_encrypt_list", ctypes.c_int,
     [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, sz, ctypes.c_double, u64p]),
    ("tfhe_mi355_debug_torus_from_fraction", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(ctypes.c_double), u64p, u64p, sz]),
    ("tfhe_mi355_debug_pbs_resident", ctypes.c_int, [vp, ctypes.POINTER(sz)]),
    ("tfhe_mi355_client_gen_seeded_bootstrap_key", ctypes.c_int,
     [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, u64p, ctypes.c_uint32]),
    ("tfhe_mi355_client_gen_seeded_keyswitch_key", ctypes.c_int,
     [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, ctypes.c_uint32,
      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, u64p]),
    ("tfhe_mi355_client_csprng_mask_words", ctypes.c_int,
     [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, sz, u64p]),
    ("tfhe_mi355_client_lwe_encrypt", ctypes.c_int,
     [ctypes.c_uint64, u64p, ctypes.c_uint32, u64p, sz, ctypes.c_double, u64p]),
    ("tfhe_mi355_client_lwe_decrypt", ctypes.c_int, [u64p, ctypes.c_uint32, u64p, sz, u64p]),
    ("tfhe_mi355_context_parameters", ctypes.c_int, [vp, ctypes.POINTER(TfheMi355Parameters)]),
    ("tfhe_mi355_compressed_server_key_inspect", ctypes.c_int, [u8p, sz, ctypes.POINTER(TfheMi355ServerKeyInfo)]),
    ("tfhe_mi355_compressed_server_key_upload", ctypes.c_int, [vp, u8p, sz]),
    ("tfhe_mi355_server_key_inspect", ctypes.c_int, [u8p, sz, ctypes.POINTER(TfheMi355ServerKeyInfo)]),
    ("tfhe_mi355_server_key_upload", ctypes.c_int, [vp, u8p, sz]),
    ("tfhe_mi355_fourier_engine_frequency", ctypes.c_int, [ctypes.c_uint32, u32p]),
    ("tfhe_mi355_kernel_timing_enable", ctypes.c_int, [vp, ctypes.c_int]),
    ("tfhe_mi355_kernel_timing_entry", ctypes.c_int,
     [vp, sz, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
    ("tfhe_mi355_submit", ctypes.c_int,
     [vp, ctypes.c_int, u64p, u64p, u64p, sz, u32p, sz, ctypes.POINTER(vp)]),
    ("tfhe_mi355_wait", ctypes.c_int, [vp]),
    ("tfhe_mi355_coalesce_stats", ctypes.c_int,
     [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
    # 32-bit torus (the reference's boolean module)
    ("tfhe_mi355_bootstrap_key_upload_u32", ctypes.c_int, [vp, u32p, sz]),
    ("tfhe_mi355_keyswitch_key_upload_u32", ctypes.c_int, [vp, u32p, sz]),
    ("tfhe_mi355_programmable_bootstrap_u32", ctypes.c_int, [vp, u32p, u32p, u32p, sz, u32p, sz]),
    ("tfhe_mi355_programmable_bootstrap_u32_async", ctypes.c_int, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_programmable_bootstrap_u32_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_blind_rotate_u32", ctypes.c_int, [vp, u32p, u32p, u32p, sz, u32p, sz]),
    ("tfhe_mi355_blind_rotate_u32_async", ctypes.c_int, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_blind_rotate_u32_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_keyswitch_u32", ctypes.c_int, [vp, u32p, u32p, sz]),
    ("tfhe_mi355_keyswitch_u32_async", ctypes.c_int, [vp, vp, vp, sz, vp, sz, vp]),
    ("tfhe_mi355_keyswitch_u32_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_boolean_gates", ctypes.c_int, [vp, u8p, u32p, u32p, u32p, sz, ctypes.c_int]),
    ("tfhe_mi355_boolean_gates_async", ctypes.c_int, [vp, vp, vp, vp, vp, sz, ctypes.c_int, vp, sz, vp]),
    ("tfhe_mi355_boolean_gates_scratch", ctypes.c_int, [vp, sz, ctypes.c_int, ctypes.POINTER(sz)]),
    ("tfhe_mi355_boolean_mux", ctypes.c_int, [vp, u32p, u32p, u32p, u32p, sz, ctypes.c_int]),
    ("tfhe_mi355_boolean_mux_async", ctypes.c_int, [vp, vp, vp, vp, vp, sz, ctypes.c_int, vp, sz, vp]),
    ("tfhe_mi355_boolean_mux_scratch", ctypes.c_int, [vp, sz, ctypes.c_int, ctypes.POINTER(sz)]),
    ("tfhe_mi355_boolean_not_async", ctypes.c_int, [vp, vp, vp, sz, vp]),
    ("tfhe_mi355_debug_torus32_from_fraction", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(ctypes.c_double), u32p, u32p, sz]),
    ("tfhe_mi355_debug_keyswitch_u32", ctypes.c_int,
     [vp, u32p, sz, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, u32p, u32p, sz]),
    ("tfhe_mi355_debug_pbs_u32_resident", ctypes.c_int, [vp, ctypes.POINTER(sz)]),
    ("tfhe_mi355_context_create_u128", ctypes.c_int,
     [ctypes.POINTER(TfheMi355Parameters), ctypes.c_int, ctypes.POINTER(vp)]),
    ("tfhe_mi355_bootstrap_key_upload_u128", ctypes.c_int, [vp, u64p, sz]),
    ("tfhe_mi355_programmable_bootstrap_u128", ctypes.c_int, [vp, u64p, u64p, u64p, sz, u32p, sz, ctypes.c_uint32]),
    ("tfhe_mi355_programmable_bootstrap_u128_async", ctypes.c_int,
     [vp, vp, vp, vp, sz, vp, sz, ctypes.c_uint32, vp, sz, vp]),
    ("tfhe_mi355_programmable_bootstrap_u128_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_blind_rotate_u128", ctypes.c_int, [vp, u64p, u64p, u64p, sz, u32p, sz, ctypes.c_uint32]),
    ("tfhe_mi355_blind_rotate_u128_async", ctypes.c_int, [vp, vp, vp, vp, sz, vp, sz, ctypes.c_uint32, vp, sz, vp]),
    ("tfhe_mi355_blind_rotate_u128_scratch", ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    ("tfhe_mi355_debug_fft128_tables", ctypes.c_int,
     [ctypes.c_uint32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    ("tfhe_mi355_debug_torus128_from_f128", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), u64p, u64p, sz]),
    ("tfhe_mi355_debug_pbs_u128_resident", ctypes.c_int, [vp, ctypes.POINTER(sz)]),
]

_lib = None


class EngineError(RuntimeError):
    """Raised when a C-ABI call returns 1 (the reference panics in the same situations)."""


def load():
    global _lib
    if _lib is not None:
        return _lib
    try:  # share torch's HIP runtime if torch is present (see module docstring)
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is always present in this image
        pass
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            f"HIP engine library not built: {LIB_PATH} (run __graft_entry__.build() or make -C "
            f"tfhe-rs-odd_amd); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.tfhe_mi355_last_error()
        raise EngineError(f"{name}: {msg.decode() if msg else 'failure'}")
