"""Integer WoP-PBS (tfhe_mi355/integer.py WopbsKey, shortint.py WopbsKey's cross-set half) without a GPU:
the LUT generators against literal values, and the execution (bit grouping, one composed call with one
output per block, the keyswitches between the PBS and the WoP set) on the CPU stand-in of the engine
(tests/integer_wopbs_cases.py).  Every comparison of ciphertexts is bit-exact.

Sets: WOPBS 2_2 and PARAM_MESSAGE_2_CARRY_2_KS_PBS with lwe_dimension cut to 96.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import integer_wopbs_cases as cases

U64 = np.uint64


def _integer():
    from tfhe_mi355 import integer

    return integer


def _lut_key():
    """A WopbsKey that only generates LUTs (no engine behind it)."""
    return _integer().WopbsKey(SimpleNamespace(param=cases.params("wop_2_2")))


def _batch(degree, K=1, words=5):
    return _integer().RadixBatch(np.zeros((K, len(degree), words), dtype=U64), list(degree), [1] * len(degree))


# ---- module functions ---------------------------------------------------------------------------------
def test_radix_helpers():
    I = _integer()
    assert I.encode_radix(11, 2, 5) == [1, 1, 0, 1, 0]
    assert I.decode_radix(I.encode_radix(11, 2, 5), 2) == 11
    assert I.encode_radix(42, 4, 3) == [2, 2, 2] and I.decode_radix([2, 2, 2], 4) == 42
    assert I.decode_radix([1, 1], 1 << 63) == (1 + (1 << 63))     # wrapping u64 arithmetic
    assert I.decode_radix([0, 0, 1], 1 << 32) == 0
    assert I.split_value_according_to_bit_basis(5, [1, 2]) == [1, 2]
    assert I.split_value_according_to_bit_basis(0b110110, [2, 1, 3]) == [2, 1, 6]
    # a 2-bit field holds its digit; a 3-bit field carries its third bit into the next digit
    assert I.encode_mix_radix(0b0111, [2, 2], 4) == [3, 1]
    assert I.encode_mix_radix(0b001111, [3, 3], 4) == [3, 2]


# ---- LUT generators against literal values ----------------------------------------------------------------
def test_generate_lut_radix_identity_three_blocks_of_degree_3():
    wk = _lut_key()
    lut = wk.generate_lut_radix(_batch([3, 3, 3]), lambda x: x)
    assert lut.shape == (3, 2048) and lut.dtype == U64          # 6 bits < log2 N: the LUT size is N
    for o in range(3):
        assert [int(v) for v in lut[o, :64]] == [((idx >> (2 * o)) & 3) << 59 for idx in range(64)]
    assert not lut[:, 64:].any()


def test_generate_lut_radix_doc_example_42_doubled():
    wk = _lut_key()
    lut = wk.generate_lut_radix(_batch([3, 3, 3]), lambda x: 2 * x)
    # 42 = (2, 2, 2) in base 4 is index 0b101010; 84 mod 64 = 20 = (0, 1, 1)
    assert [int(lut[o, 42]) >> 59 for o in range(3)] == [0, 1, 1]
    assert [int(lut[o, 63]) >> 59 for o in range(3)] == [2, 3, 3]  # 126 mod 64 = 62


def test_generate_lut_radix_mixed_degrees_use_5_bits():
    wk = _lut_key()
    lut = wk.generate_lut_radix(_batch([3, 1, 3]), lambda x: x)
    assert lut.shape == (3, 2048)
    assert lut[:, :32].any() and not lut[:, 32:].any()
    # index bits (low to high): 2 of block 0, 1 of block 1, 2 of block 2.  Block 1 = 1, the others 0:
    assert [int(lut[o, 0b00100]) >> 59 for o in range(3)] == [0, 1, 0]
    assert [int(lut[o, 0b01011]) >> 59 for o in range(3)] == [3, 2, 0]   # blocks (3, 0, 1): digit 1 reads 2 bits
    deg7 = wk.generate_lut_radix(_batch([7, 3]), lambda x: x)            # degree 7: 3 bits, the third a carry
    assert [int(deg7[o, 0b00111]) >> 59 for o in range(2)] == [3, 1]
    assert [int(deg7[o, 0b11111]) >> 59 for o in range(2)] == [3, 0]     # 3 + 4 (1 + 3) = 19 mod 16 = 3


def test_generate_lut_radix_without_padding_folds_the_carry_bits():
    wk = _lut_key()
    lut = wk.generate_lut_radix_without_padding(_batch([3, 3, 3]), lambda x: x)
    assert lut.shape == (3, 4096)                                         # 3 blocks x 4 bits = 12 bits
    # message bits only: index 0x213 is blocks (3, 1, 2) = 3 + 4 + 32
    assert [int(lut[o, 0x213]) >> 60 for o in range(3)] == [3, 1, 2]
    # carry bits of block 0 (0xC: carry 3) land on block 1's message bits: value 3 << 2 = 12 = (0, 3, 0)
    assert [int(lut[o, 0x00C]) >> 60 for o in range(3)] == [0, 3, 0]
    # block 0 = 7 (message 3, carry 1), block 1 = 5 (message 1, carry 1): 7 + 5 * 4 = 27 = (3, 2, 1)
    assert [int(lut[o, 0x057]) >> 60 for o in range(3)] == [3, 2, 1]
    doubled = wk.generate_lut_radix_without_padding(_batch([3, 3, 3]), lambda x: 2 * x)
    assert [int(doubled[o, 0x033]) >> 60 for o in range(3)] == [2, 3, 1]  # 15 -> 30 = (2, 3, 1)
    one = wk.generate_lut_radix_without_padding(_batch([3]), lambda x: x)
    assert one.shape == (1, 2048) and [int(v) >> 60 for v in one[0, :16]] == [i % 4 for i in range(16)]
    assert [int(v) >> 60 for v in one[0, 16:32]] == [i % 4 for i in range(16)]   # filled over the whole size


def test_generate_lut_bivariate_radix_splits_at_the_first_operands_bits():
    wk = _lut_key()
    a, b = _batch([3, 3]), _batch([3, 1])
    lut = wk.generate_lut_bivariate_radix(a, b, lambda x, y: x + 3 * y)
    assert lut.shape == (2, 2048)                                         # 4 + 3 = 7 bits, two outputs
    assert lut[:, :128].any() and not lut[:, 128:].any()
    for idx in (0b0001011, 0b1100110, 0b1111111):
        x, y = idx & 15, idx >> 4                                         # the split at nb_bit_to_extract[0] = 4
        ydec = (y & 3) + 4 * (y >> 2)
        want = (x + 3 * ydec) % 16
        assert [int(lut[o, idx]) >> 59 for o in range(2)] == [want % 4, want // 4], idx


# ---- execution on the stand-in ------------------------------------------------------------------------------
K = 2
VALUES = np.array([27, 54], dtype=U64)   # (3, 2, 1) and (2, 1, 3) in base 4


def _wop_integer_client(wk, blocks=3):
    return _integer().ClientKey(wk.wopbs_key._wopbs_client_key, blocks)


def test_wopbs_with_padding_on_the_stand_in(orc):
    cks, wk = cases.standin_only_for_wopbs("wop_2_2")
    ick = _wop_integer_client(wk)
    ct = ick.encrypt(VALUES)
    lut = wk.generate_lut_radix(ct, lambda x: 2 * x + 1)
    res = wk.wopbs(ct, lut)
    ref, p = wk.wopbs_key.engine.ref, wk.param
    bits = cases.hand_bits(ref, ct.data, [2, 2, 2], 59)
    assert bits.shape == (K, 6, p.lwe_dimension + 1)
    exp = ref.circuit_bootstrap_vertical_packing(bits, p.cbs_base_log, p.cbs_level, lut.reshape(1, 3, 1, -1))
    assert res.data.shape == (K, 3, p.big_lwe_dimension + 1)
    assert np.array_equal(res.data, exp)
    assert res.degree == [3, 3, 3] and res.noise == [1, 1, 1]
    assert np.array_equal(ick.decrypt(res), (2 * VALUES + 1) % 64)


def test_wopbs_groups_blocks_by_bit_count_and_skips_degree_0(orc):
    """degrees [3, 1, 0]: one extract_bits call for the 2-bit block, one for the 1-bit block, none for the
    block of degree 0; 3 bits in all, most significant block first."""
    cks, wk = cases.standin_only_for_wopbs("wop_2_2")
    I = _integer()
    ick = _wop_integer_client(wk)
    ct = ick.encrypt(np.array([3 + 4 * 1, 2 + 4 * 0], dtype=U64))
    ct.data[:, 2, :] = 0
    ct.degree = [3, 1, 0]
    eng = wk.wopbs_key.engine
    seen = []
    real = eng.extract_bits
    eng.extract_bits = lambda x, d, n: (seen.append((np.asarray(x).shape[0], d, n)), real(x, d, n))[1]
    try:
        lut = wk.generate_lut_radix(ct, lambda x: x + 1)
        res = wk.wopbs(ct, lut)
    finally:
        del eng.extract_bits
    assert sorted(seen) == [(K, 59, 1), (K, 59, 2)]
    p = wk.param
    bits = cases.hand_bits(eng.ref, ct.data, [2, 1, 0], 59)
    assert bits.shape[1] == 3
    exp = eng.ref.circuit_bootstrap_vertical_packing(bits, p.cbs_base_log, p.cbs_level, lut.reshape(1, 3, 1, -1))
    assert np.array_equal(res.data, exp)
    assert np.array_equal(ick.decrypt(res), [8, 3])
    with pytest.raises(ValueError, match="no bit to extract"):
        wk.wopbs(I.RadixBatch(ct.data, [0, 0, 0], [1, 1, 1]), lut)
    with pytest.raises(ValueError, match="LUT must be"):
        wk.wopbs(ct, lut[:, :1024])


def test_wopbs_without_padding_on_the_stand_in(orc):
    cks, wk = cases.standin_only_for_wopbs("wop_2_2")
    ick = _wop_integer_client(wk)
    ct = ick.encrypt_without_padding(VALUES)
    lut = wk.generate_lut_radix_without_padding(ct, lambda x: 2 * x)
    res = wk.wopbs_without_padding(ct, lut)
    ref, p = wk.wopbs_key.engine.ref, wk.param
    bits = cases.hand_bits(ref, ct.data, [4, 4, 4], 60)
    assert bits.shape == (K, 12, p.lwe_dimension + 1)
    exp = ref.circuit_bootstrap_vertical_packing(bits, p.cbs_base_log, p.cbs_level, lut.reshape(1, 3, 2, -1))
    assert np.array_equal(res.data, exp)
    assert np.array_equal(ick.decrypt_without_padding(res), (2 * VALUES) % 64)


def test_bivariate_wopbs_with_degree_on_the_stand_in(orc):
    cks, wk = cases.standin_only_for_wopbs("wop_2_2")
    ick = _wop_integer_client(wk)
    other = np.array([5, 62], dtype=U64)
    ct1, ct2 = ick.encrypt(VALUES), ick.encrypt(other)
    lut = wk.generate_lut_bivariate_radix(ct1, ct2, lambda x, y: 2 * x * y)
    assert lut.shape == (3, 4096)
    res = wk.bivariate_wopbs_with_degree(ct1, ct2, lut)
    ref, p = wk.wopbs_key.engine.ref, wk.param
    both = np.concatenate([ct1.data, ct2.data], axis=1)
    bits = cases.hand_bits(ref, both, [2] * 6, 59)
    exp = ref.circuit_bootstrap_vertical_packing(bits, p.cbs_base_log, p.cbs_level, lut.reshape(1, 3, 2, -1))
    assert res.num_blocks == 3                                            # the first len(ct1) outputs
    assert np.array_equal(res.data, exp)
    assert np.array_equal(ick.decrypt(res), (2 * VALUES * other) % 64)


# ---- the keyswitches between the PBS and the WoP set ----------------------------------------------------------
def test_only_for_wopbs_key_has_no_way_into_the_wop_set(orc):
    cks, wk = cases.standin_only_for_wopbs("wop_2_2")
    ct = _wop_integer_client(wk).encrypt(VALUES)
    with pytest.raises(ValueError, match="only for wopbs"):
        wk.keyswitch_to_wopbs_params(wk.wopbs_key.wopbs_server_key, ct)
    with pytest.raises(ValueError, match="only for wopbs"):
        wk.wopbs_key.keyswitch_to_wopbs_params(wk.wopbs_key.wopbs_server_key, cks.encrypt(1))
    back = wk.keyswitch_to_pbs_params(ct)                                 # the same set: its own KS and PBS
    assert np.array_equal(_wop_integer_client(wk).decrypt(back), VALUES)
    assert wk.wopbs_key.engine.ks_calls == []


def test_cross_set_round_trip_on_the_stand_in(orc):
    """PBS -> WoP -> wopbs -> PBS decrypts under the original client key; the two cross keyswitches run
    with the cross keys' dimensions (PBS big -> WoP big on the WoP engine, WoP big -> PBS small on the PBS
    engine), both with the PBS set's decomposition, one call each over every block."""
    I = _integer()
    cks, sks, wk = cases.standin_cross()
    wop_eng, pbs_eng = wk.wopbs_key.engine, sks.engine
    assert wop_eng is not pbs_eng and wk.wopbs_key.pbs_server_key is sks
    wcks = wk.wopbs_key._wopbs_client_key
    assert not np.array_equal(wcks.glwe_secret_key, cks.glwe_secret_key)  # keys of the WoP set's own
    del wop_eng.ks_calls[:], pbs_eng.ks_calls[:]
    ick = I.ClientKey(cks, 3)
    ct = ick.encrypt(VALUES)
    ct.degree = [3, 3, 2]
    wct = wk.keyswitch_to_wopbs_params(sks, ct)
    pp, wp = cks.parameters, wk.param
    assert wop_eng.ks_calls == [(pp.big_lwe_dimension, wp.big_lwe_dimension, pp.ks_base_log, pp.ks_level, 3 * K)]
    assert wct.degree == [3, 3, 2] and wct.noise == [1, 1, 1]             # the degrees are kept
    assert wct.data.shape == (K, 3, wp.big_lwe_dimension + 1)
    assert np.array_equal(I.ClientKey(wcks, 3).decrypt(wct), VALUES)      # under the WoP set's key now
    res = wk.wopbs(wct, wk.generate_lut_radix(wct, lambda x: 2 * x))
    out = wk.keyswitch_to_pbs_params(res)
    assert pbs_eng.ks_calls == [(wp.big_lwe_dimension, pp.lwe_dimension, pp.ks_base_log, pp.ks_level, 3 * K)]
    assert out.degree == [3, 3, 3]
    assert np.array_equal(ick.decrypt(out), (2 * VALUES) % 64)
    # the shortint forms: one ciphertext, and a list as one batch
    blocks = cks.encrypt_many([1, 2, 3])
    del wop_eng.ks_calls[:]
    sw = wk.wopbs_key
    moved = sw.keyswitch_to_wopbs_params(sks, blocks)
    assert [c[4] for c in wop_eng.ks_calls] == [3]
    lut = sw.generate_lut(moved[0], lambda x: (3 * x) % 4)
    back = sw.keyswitch_to_pbs_params(sw.wopbs(moved, lut))
    assert [cks.decrypt(c) for c in back] == [3, 2, 1]
    assert cks.decrypt(sw.programmable_bootstrapping(sks, blocks[2], lut)) == 1
    bits = sw.extract_bits(59, moved[1], 4)
    assert bits.shape == (4, wp.lwe_dimension + 1)
    one = sw.circuit_bootstrapping_vertical_packing(np.stack([lut, lut]), bits)
    assert one.shape == (2, wp.big_lwe_dimension + 1) and np.array_equal(one[0], one[1])
