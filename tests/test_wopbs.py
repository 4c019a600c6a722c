"""The bootstrapped half of WoP-PBS without a GPU: the parameter sets' reference constants, the client-
side pfpksk generator checked by the phase of the reference pfpks (tests/wopbs_reference.py, built
from the oracle), the reference chain decrypting the fixed inputs the GPU decryption test uses, and
the Python-side validation errors."""
import numpy as np
import pytest

from ggsw_reference import Ref, lut_value, torus_distance
from wopbs_reference import decrypt_case, pfpks, pfpksk_shape

U64 = np.uint64


def test_wopbs_parameter_sets_match_reference_constants():
    from tfhe_mi355 import parameters as P

    def fields(p):
        return (p.lwe_dimension, p.glwe_dimension, p.polynomial_size, p.pbs_base_log, p.pbs_level, p.ks_base_log,
                p.ks_level, p.pfks_base_log, p.pfks_level, p.cbs_base_log, p.cbs_level, p.message_modulus,
                p.carry_modulus)

    assert fields(P.WOPBS_PARAM_MESSAGE_1_CARRY_1_KS_PBS) == (653, 1, 2048, 15, 2, 5, 2, 15, 2, 5, 3, 2, 2)
    assert fields(P.WOPBS_PARAM_MESSAGE_1_CARRY_2_KS_PBS) == (487, 3, 512, 9, 3, 2, 4, 9, 3, 3, 5, 2, 4)
    assert fields(P.WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS) == (769, 1, 2048, 15, 2, 6, 2, 15, 2, 5, 3, 4, 4)
    p = P.WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS
    assert (p.lwe_modular_std_dev, p.glwe_modular_std_dev, p.pfks_modular_std_dev) == (
        0.0000043131554647504185, 0.00000000000000029403601535432533, 0.00000000000000029403601535432533)
    assert P.WOPBS_PARAM_MESSAGE_1_CARRY_2_KS_PBS.pfks_modular_std_dev == 0.000000000002573000821792597679153983627
    assert P.WOPBS_PARAM_MESSAGE_1_CARRY_1_KS_PBS.lwe_modular_std_dev == 0.00003604499526942373
    assert isinstance(p, P.ClassicPBSParameters) and p.encryption_key_choice == "Big" and p.delta == 1 << 59
    assert p.with_(lwe_dimension=96).cbs_level == 3  # with_ keeps the WoP fields


@pytest.mark.parametrize("N,k,B,L,std", [(2048, 1, 15, 2, 2.94036015354e-16), (512, 3, 9, 3, 2.5730008218e-12)])
def test_client_pfpksk_list_is_valid(orc, N, k, B, L, std):
    """The reference pfpks of an encryption of mu under key g has phase -P_g mu: +mu at the body's constant
    term for g = k, -S_g mu for g < k.

    Bound 2^48.  The pfpks is taken on the input rounded to B L bits, an error uniform in +-2^(63 - B L)
    per word; through the phase it meets the body and about kN / 2 key bits, and mu being a constant each
    output coefficient holds one such sum: std <= 2^(63 - B L) sqrt((kN/2 + 1) / 3) = 2^37.2 at (15, 2),
    2^40.0 at (9, 3).  The key noise adds (kN + 1) L terms of digit (rms 2^(B-1) / sqrt 3) x noise: 2^32.1
    and 2^39.6.  2^48 is more than 8 standard deviations of either."""
    from tfhe_mi355 import client

    sk = client.gen_binary_key(31 + N, 2, k * N)
    keys = client.gen_pfpksk_list(32 + N, sk, sk, k, N, B, L, std, threads=8)
    assert keys.size == int(np.prod(pfpksk_shape(k, N, L)))
    mus = np.array([1 << 62, 3 << 60, (1 << 64) - (5 << 59)], dtype=U64)
    cts = client.lwe_encrypt(33, sk, mus, std)
    out = pfpks(orc, keys, k, N, B, L, cts)
    ref = Ref(orc, k, N, B, L)
    S = sk.reshape(k, N)
    worst = 0.0
    for c, mu in enumerate(mus):
        for g in range(k + 1):
            ph = ref.phase(sk, out[c, g])
            if g == k:
                want = np.zeros(N, dtype=U64)
                want[0] = mu
            else:
                want = U64(0) - S[g] * mu
            worst = max(worst, torus_distance(ph, want).max())
    print(f"(N, k, B, L) = {(N, k, B, L)}: max phase error 2^{np.log2(max(worst, 1.0)):.1f}, bound 2^48")
    assert worst < 2.0 ** 48


def test_reference_chain_decrypts_at_wopbs_2_2(orc):
    """extract_bits -> circuit bootstrap -> vertical packing on the CPU reference, WOPBS 2_2 with its
    real keys, the seeds and inputs of the GPU decryption test: every message decrypts (error against
    the half step 2^59 printed)."""
    c = decrypt_case(orc)
    cks = c["cks"]
    dec = cks.decrypt_message_and_carry_without_padding_many
    from tfhe_mi355.shortint import Ciphertext

    def wrap(rows):
        return [Ciphertext(r, 3, 1, 4, 4, "KeyswitchBootstrap") for r in rows]

    # the extracted bits are the message bits, most significant first, at q/2
    raw = orc.lwe_decrypt(cks.small_lwe_secret_key, c["bits_a"].reshape(-1, c["P"].lwe_dimension + 1)).reshape(16, 4)
    bits = ((raw + U64(1 << 62)) >> U64(63)).astype(int)
    assert np.array_equal(bits, [[(m >> (3 - b)) & 1 for b in range(4)] for m in range(16)])
    got_a = dec(wrap(c["out_a"][:, 0]))
    assert np.array_equal(got_a, [lut_value(m % 4) for m in range(16)])
    got_b = dec(wrap(c["out_b"][:, 0]))
    assert np.array_equal(got_b, [lut_value(i) for i in c["index_b"]])
    pts = orc.lwe_decrypt(cks.large_lwe_secret_key, np.concatenate([c["out_a"][:, 0], c["out_b"][:, 0]]))
    want = np.array([lut_value(m % 4) for m in range(16)] + [lut_value(i) for i in c["index_b"]], dtype=U64) << U64(60)
    err = torus_distance(pts, want).max()
    print(f"max decryption error 2^{np.log2(err):.1f} against the half step 2^59")
    assert err < 2.0 ** 59


def test_python_side_validation_errors():
    from tfhe_mi355 import core_crypto as cc
    from tfhe_mi355 import parameters as P
    from tfhe_mi355.shortint import ClientKey, WopbsKey

    with pytest.raises(ValueError, match="WopbsParameters"):
        WopbsKey(None, P.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    with pytest.raises(ValueError, match="no WopbsParameters"):
        WopbsKey.new_wopbs_key_only_for_wopbs(ClientKey(P.PARAM_MESSAGE_2_CARRY_2_KS_PBS.with_(lwe_dimension=8), 1), None)
    with pytest.raises(ValueError, match="5 or 6 levels"):
        WopbsKey(None, P.WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS.with_(pbs_level=5))

    class FakeEngine:
        params = P.WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS.with_(lwe_dimension=96)
        n, big_dim = 96, 2048

    eng = FakeEngine()
    with pytest.raises(ValueError, match="expected"):
        cc.LwePrivateFunctionalPackingKeyswitchKeyList(np.zeros(10, dtype=U64), 2048, 2, 2048, 15, 2, eng)
    bsk, ksk = cc.FourierLweBootstrapKey(eng), cc.LweKeyswitchKey(eng)
    big, small = np.zeros(2049, dtype=U64), np.zeros((4, 97), dtype=U64)
    with pytest.raises(ValueError, match="maximum number of extractable"):
        cc.extract_bits_from_lwe_ciphertext(big, small, bsk, ksk, 61, 4)
    with pytest.raises(ValueError, match="lwe_in needs"):
        cc.extract_bits_from_lwe_ciphertext(big[:-1], small, bsk, ksk, 60, 4)
    with pytest.raises(ValueError, match="lwe_list_out needs to have an LWE dimension"):
        cc.extract_bits_from_lwe_ciphertext(big, np.zeros((4, 98), dtype=U64), bsk, ksk, 60, 4)
    with pytest.raises(ValueError, match="ciphertext count of 4"):
        cc.extract_bits_from_lwe_ciphertext(big, small[:3], bsk, ksk, 60, 4)
    with pytest.raises(ValueError, match="different engines"):
        cc.extract_bits_from_lwe_ciphertext(big, small, bsk, cc.LweKeyswitchKey(FakeEngine()), 60, 4)
