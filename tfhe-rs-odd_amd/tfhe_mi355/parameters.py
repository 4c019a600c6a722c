"""Parameter sets of the reference (values copied from the reference's constants; the names are
authoritative -- see SURVEY.md 0.4 for the BASELINE.json annotation mismatch).

  PARAM_MESSAGE_<m>_CARRY_<c>_{KS_PBS,PBS_KS}   shortint/parameters/mod.rs:598-1201 (every set; table below)
  PARAM_MESSAGE_<m>_CARRY_<c>_COMPACT_PK_{KS_PBS,PBS_KS}   shortint/parameters/parameters_compact_pk.rs (all 56:
                                   COMPACT_PK_ALL, the accepted ones; COMPACT_PK_REFUSED, the others)
  PARAM_MESSAGE_2_CARRY_2_KS_PBS   shortint/parameters/mod.rs:703-717 (alias :1256)
  PARAM_MESSAGE_4_CARRY_4_KS_PBS   shortint/parameters/mod.rs:1063-1077 (alias :1271)
  PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS   shortint/parameters/multi_bit.rs:173-190
  PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS   shortint/parameters/multi_bit.rs:115-132
  PARAM_MULTI_BIT_MESSAGE_{1_CARRY_1,3_CARRY_3}_GROUP_{2,3}_KS_PBS   multi_bit.rs:96-114,134-153,154-172,192-210
  MANTICORE_PARAMETERS (fork)      gadget/parameters/mod.rs:224-235
  GADGET_* (fork)                  gadget/parameters/mod.rs:84-222 (DEFAULT, SIMON_40,
                                   ZAMA_TRIVIUM, ASCON_40, SHA3_40, AES_40, AES_23, TFHE_LIB)
  TEST_PARAMS_4_BITS_NATIVE_U64    core_crypto/algorithms/test/mod.rs:56-73
  BOOLEAN_* (32-bit torus)         boolean/parameters/mod.rs:123-192 (the five BooleanParameters sets)
"""
from __future__ import annotations

from dataclasses import dataclass, replace


@dataclass(frozen=True)
class ClassicPBSParameters:
    """Mirror of shortint ClassicPBSParameters (shortint/parameters/mod.rs:60-75)."""

    lwe_dimension: int
    glwe_dimension: int
    polynomial_size: int
    lwe_modular_std_dev: float
    glwe_modular_std_dev: float
    pbs_base_log: int
    pbs_level: int
    ks_base_log: int
    ks_level: int
    message_modulus: int
    carry_modulus: int
    encryption_key_choice: str = "Big"  # "Big" = KS -> PBS order (PBSOrder::KeyswitchBootstrap)
    grouping_factor: int = 0            # > 0: MultiBitPBSParameters
    name: str = ""

    @property
    def big_lwe_dimension(self) -> int:
        return self.glwe_dimension * self.polynomial_size

    @property
    def delta(self) -> int:
        return (1 << 63) // (self.message_modulus * self.carry_modulus)

    def with_(self, **kw) -> "ClassicPBSParameters":
        return replace(self, **kw)


PARAM_MESSAGE_2_CARRY_2_KS_PBS = ClassicPBSParameters(
    lwe_dimension=742, glwe_dimension=1, polynomial_size=2048,
    lwe_modular_std_dev=0.000007069849454709433,
    glwe_modular_std_dev=0.00000000000000029403601535432533,
    pbs_base_log=23, pbs_level=1, ks_base_log=3, ks_level=5,
    message_modulus=4, carry_modulus=4, name="PARAM_MESSAGE_2_CARRY_2_KS_PBS")
PARAM_MESSAGE_2_CARRY_2 = PARAM_MESSAGE_2_CARRY_2_KS_PBS

PARAM_MESSAGE_4_CARRY_4_KS_PBS = ClassicPBSParameters(
    lwe_dimension=996, glwe_dimension=1, polynomial_size=32768,
    lwe_modular_std_dev=0.00000006767666038309478,
    glwe_modular_std_dev=0.0000000000000000002168404344971009,
    pbs_base_log=15, pbs_level=2, ks_base_log=3, ks_level=7,
    message_modulus=16, carry_modulus=16, name="PARAM_MESSAGE_4_CARRY_4_KS_PBS")
PARAM_MESSAGE_4_CARRY_4 = PARAM_MESSAGE_4_CARRY_4_KS_PBS

PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS = ClassicPBSParameters(
    lwe_dimension=888, glwe_dimension=1, polynomial_size=2048,
    lwe_modular_std_dev=0.0000006125031601933181,
    glwe_modular_std_dev=0.0000000000000003152931493498455,
    pbs_base_log=21, pbs_level=1, ks_base_log=7, ks_level=2,
    message_modulus=4, carry_modulus=4, grouping_factor=3,
    name="PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS")

PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS = ClassicPBSParameters(
    lwe_dimension=818, glwe_dimension=1, polynomial_size=2048,
    lwe_modular_std_dev=0.000002226459789930014,
    glwe_modular_std_dev=0.0000000000000003152931493498455,
    pbs_base_log=22, pbs_level=1, ks_base_log=5, ks_level=3,
    message_modulus=4, carry_modulus=4, grouping_factor=2,
    name="PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS")

# the other multi-bit sets (shortint/parameters/multi_bit.rs:96-153, 154-210)
PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS = ClassicPBSParameters(
    lwe_dimension=764, glwe_dimension=3, polynomial_size=512,
    lwe_modular_std_dev=0.000006025673585415336, glwe_modular_std_dev=0.0000000000039666089171633006,
    pbs_base_log=18, pbs_level=1, ks_base_log=6, ks_level=2, message_modulus=2, carry_modulus=2,
    grouping_factor=2, name="PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS")
PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS = ClassicPBSParameters(
    lwe_dimension=922, glwe_dimension=1, polynomial_size=8192,
    lwe_modular_std_dev=0.0000003272369292345697, glwe_modular_std_dev=0.0000000000000000002168404344971009,
    pbs_base_log=14, pbs_level=2, ks_base_log=4, ks_level=4, message_modulus=8, carry_modulus=8,
    grouping_factor=2, name="PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS")
PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS = ClassicPBSParameters(
    lwe_dimension=765, glwe_dimension=3, polynomial_size=512,
    lwe_modular_std_dev=0.000005915594083804978, glwe_modular_std_dev=0.0000000000039666089171633006,
    pbs_base_log=18, pbs_level=1, ks_base_log=6, ks_level=2, message_modulus=2, carry_modulus=2,
    grouping_factor=3, name="PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS")
PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS = ClassicPBSParameters(
    lwe_dimension=972, glwe_dimension=1, polynomial_size=8192,
    lwe_modular_std_dev=0.00000013016688349592805, glwe_modular_std_dev=0.0000000000000000002168404344971009,
    pbs_base_log=14, pbs_level=2, ks_base_log=6, ks_level=3, message_modulus=8, carry_modulus=8,
    grouping_factor=3, name="PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS")
MULTI_BIT_ALL = {p.name: p for p in [
    PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS, PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS,
    PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS, PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS,
    PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS, PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS]}

# fork: GadgetParameters carry no message/carry moduli; 2 x 2 used here for LUT boxes
MANTICORE_PARAMETERS = ClassicPBSParameters(
    lwe_dimension=754, glwe_dimension=1, polynomial_size=1024,
    lwe_modular_std_dev=8.829486224734387e-11,
    glwe_modular_std_dev=5.871712650082723e-15,
    pbs_base_log=15, pbs_level=2, ks_base_log=4, ks_level=3,
    message_modulus=2, carry_modulus=2, name="MANTICORE_PARAMETERS")



def _gadget(name, n, k, N, lwe_std, glwe_std, pbs_bl, pbs_l, ks_bl, ks_l, choice):
    return ClassicPBSParameters(lwe_dimension=n, glwe_dimension=k, polynomial_size=N, lwe_modular_std_dev=lwe_std,
                                glwe_modular_std_dev=glwe_std, pbs_base_log=pbs_bl, pbs_level=pbs_l,
                                ks_base_log=ks_bl, ks_level=ks_l, message_modulus=2, carry_modulus=2,
                                encryption_key_choice=choice, name=name)


# the fork's other GadgetParameters (k = 2, 3, 5 at N = 256..1024)
GADGET_DEFAULT_PARAMETERS = _gadget("GADGET_DEFAULT_PARAMETERS", 722, 2, 512, 0.000013071021089943935,
                                    0.00000004990272175010415, 6, 3, 3, 4, "Small")
GADGET_SIMON_PARAMETERS_40 = _gadget("GADGET_SIMON_PARAMETERS_40", 684, 3, 512, 1.52587890625e-05,
                                     9.313225746154785e-10, 10, 2, 3, 4, "Big")
GADGET_ZAMA_TRIVIUM_PARAMETERS = _gadget("GADGET_ZAMA_TRIVIUM_PARAMETERS", 684, 3, 512, 0.0000204378,
                                         0.000000000000345253, 18, 1, 4, 3, "Small")
GADGET_ASCON_PARAMETERS_40 = _gadget("GADGET_ASCON_PARAMETERS_40", 740, 2, 1024, 1.9073486328125e-06,
                                     9.313225746154785e-10, 7, 3, 5, 3, "Big")
GADGET_SHA3_PARAMETERS_40 = _gadget("GADGET_SHA3_PARAMETERS_40", 676, 5, 256, 0.0009765625,
                                    0.0000000000000000008673617379884035, 14, 1, 4, 3, "Big")
GADGET_AES_PARAMETERS_40 = _gadget("GADGET_AES_PARAMETERS_40", 708, 3, 512, 3.0517578125e-05,
                                   9.313225746154785e-10, 6, 4, 2, 7, "Big")
GADGET_AES_PARAMETERS_23 = _gadget("GADGET_AES_PARAMETERS_23", 672, 3, 512, 0.0000000010797982869590127,
                                   0.0000000000000000008673617379884035, 7, 3, 3, 4, "Big")
GADGET_TFHE_LIB_PARAMETERS = _gadget("GADGET_TFHE_LIB_PARAMETERS", 830, 2, 1024, 0.000001412290588219445,
                                     0.00000000000000029403601535432533, 23, 1, 5, 3, "Small")
GADGET_ALL = [GADGET_DEFAULT_PARAMETERS, GADGET_SIMON_PARAMETERS_40, GADGET_ZAMA_TRIVIUM_PARAMETERS,
              GADGET_ASCON_PARAMETERS_40, GADGET_SHA3_PARAMETERS_40, GADGET_AES_PARAMETERS_40,
              GADGET_AES_PARAMETERS_23, GADGET_TFHE_LIB_PARAMETERS]

TEST_PARAMS_4_BITS_NATIVE_U64 = PARAM_MESSAGE_2_CARRY_2_KS_PBS.with_(name="TEST_PARAMS_4_BITS_NATIVE_U64")

# The two sets of the reference's f128 PBS test (algorithms/test/lwe_programmable_bootstrapping.rs:169-205):
# u128 words, message_modulus = 2^message_modulus_log with one bit of padding; the second set computes
# modulo 2^127 (Engine.programmable_bootstrap_u128(..., ciphertext_modulus_log=127)).
TEST_PARAMS_4_BITS_NATIVE_U128 = ClassicPBSParameters(
    lwe_dimension=742, glwe_dimension=1, polynomial_size=2048, lwe_modular_std_dev=4.9982771e-11,
    glwe_modular_std_dev=8.6457178e-32, pbs_base_log=23, pbs_level=1, ks_base_log=3, ks_level=5,
    message_modulus=16, carry_modulus=1, name="TEST_PARAMS_4_BITS_NATIVE_U128")
TEST_PARAMS_3_BITS_127_U128 = TEST_PARAMS_4_BITS_NATIVE_U128.with_(message_modulus=8,
                                                                   name="TEST_PARAMS_3_BITS_127_U128")
U128_CIPHERTEXT_MODULUS_LOG = {"TEST_PARAMS_4_BITS_NATIVE_U128": 128, "TEST_PARAMS_3_BITS_127_U128": 127}

# Every shortint ClassicPBSParameters set of the reference (shortint/parameters/mod.rs:598-1201):
# (name, source line, n, k, N, lwe std, glwe std, pbs base_log, pbs level, ks base_log, ks level,
#  message modulus, carry modulus, encryption key choice)
_SHORTINT_TABLE = [
    ("PARAM_MESSAGE_1_CARRY_0_KS_PBS", 598, 678, 5, 256, 0.000022810107419132102, 0.00000000037411618952047216,
     15, 1, 5, 2, 2, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_1_KS_PBS", 613, 684, 3, 512, 0.00002043784477291318, 0.0000000000034525330484572114,
     18, 1, 4, 3, 2, 2, "Big"),
    ("PARAM_MESSAGE_2_CARRY_0_KS_PBS", 628, 656, 2, 512, 0.000034119201269311964, 0.00000004053919869756513,
     8, 2, 3, 4, 4, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_2_KS_PBS", 643, 742, 2, 1024, 0.000007069849454709433, 0.00000000000000029403601535432533,
     23, 1, 4, 3, 2, 4, "Big"),
    ("PARAM_MESSAGE_2_CARRY_1_KS_PBS", 658, 742, 2, 1024, 0.000007069849454709433, 0.00000000000000029403601535432533,
     23, 1, 4, 3, 4, 2, "Big"),
    ("PARAM_MESSAGE_3_CARRY_0_KS_PBS", 673, 742, 2, 1024, 0.000007069849454709433, 0.00000000000000029403601535432533,
     23, 1, 4, 3, 8, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_3_KS_PBS", 688, 745, 1, 2048, 0.000006692125069956277, 0.00000000000000029403601535432533,
     23, 1, 3, 5, 2, 8, "Big"),
    ("PARAM_MESSAGE_2_CARRY_2_KS_PBS", 703, 742, 1, 2048, 0.000007069849454709433, 0.00000000000000029403601535432533,
     23, 1, 3, 5, 4, 4, "Big"),
    ("PARAM_MESSAGE_3_CARRY_1_KS_PBS", 718, 742, 1, 2048, 0.000007069849454709433, 0.00000000000000029403601535432533,
     23, 1, 3, 5, 8, 2, "Big"),
    ("PARAM_MESSAGE_4_CARRY_0_KS_PBS", 733, 742, 1, 2048, 0.000007069849454709433, 0.00000000000000029403601535432533,
     23, 1, 3, 5, 16, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_4_KS_PBS", 748, 807, 1, 4096, 0.0000021515145918907506, 0.0000000000000000002168404344971009,
     15, 2, 3, 5, 2, 16, "Big"),
    ("PARAM_MESSAGE_2_CARRY_3_KS_PBS", 763, 856, 1, 4096, 0.0000008775214009854235, 0.0000000000000000002168404344971009,
     22, 1, 3, 6, 4, 8, "Big"),
    ("PARAM_MESSAGE_3_CARRY_2_KS_PBS", 778, 812, 1, 4096, 0.0000019633637461248447, 0.0000000000000000002168404344971009,
     22, 1, 3, 5, 8, 4, "Big"),
    ("PARAM_MESSAGE_4_CARRY_1_KS_PBS", 793, 808, 1, 4096, 0.0000021124945159091033, 0.0000000000000000002168404344971009,
     22, 1, 3, 5, 16, 2, "Big"),
    ("PARAM_MESSAGE_5_CARRY_0_KS_PBS", 808, 807, 1, 4096, 0.0000021515145918907506, 0.0000000000000000002168404344971009,
     22, 1, 3, 5, 32, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_5_KS_PBS", 823, 864, 1, 8192, 0.000000757998020150446, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 2, 32, "Big"),
    ("PARAM_MESSAGE_2_CARRY_4_KS_PBS", 838, 864, 1, 8192, 0.000000757998020150446, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 4, 16, "Big"),
    ("PARAM_MESSAGE_3_CARRY_3_KS_PBS", 853, 864, 1, 8192, 0.000000757998020150446, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 8, 8, "Big"),
    ("PARAM_MESSAGE_4_CARRY_2_KS_PBS", 868, 864, 1, 8192, 0.000000757998020150446, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 16, 4, "Big"),
    ("PARAM_MESSAGE_5_CARRY_1_KS_PBS", 883, 875, 1, 8192, 0.0000006197725091905067, 0.0000000000000000002168404344971009,
     22, 1, 3, 6, 32, 2, "Big"),
    ("PARAM_MESSAGE_6_CARRY_0_KS_PBS", 898, 915, 1, 8192, 0.00000029804653749339636, 0.0000000000000000002168404344971009,
     22, 1, 4, 4, 64, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_6_KS_PBS", 913, 930, 1, 16384, 0.00000022649232786295453, 0.0000000000000000002168404344971009,
     11, 3, 3, 6, 2, 64, "Big"),
    ("PARAM_MESSAGE_2_CARRY_5_KS_PBS", 928, 934, 1, 16384, 0.00000021050318566634375, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 4, 32, "Big"),
    ("PARAM_MESSAGE_3_CARRY_4_KS_PBS", 943, 930, 1, 16384, 0.00000022649232786295453, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 8, 16, "Big"),
    ("PARAM_MESSAGE_4_CARRY_3_KS_PBS", 958, 930, 1, 16384, 0.00000022649232786295453, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 16, 8, "Big"),
    ("PARAM_MESSAGE_5_CARRY_2_KS_PBS", 973, 930, 1, 16384, 0.00000022649232786295453, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 32, 4, "Big"),
    ("PARAM_MESSAGE_6_CARRY_1_KS_PBS", 988, 930, 1, 16384, 0.00000022649232786295453, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 64, 2, "Big"),
    ("PARAM_MESSAGE_7_CARRY_0_KS_PBS", 1003, 930, 1, 16384, 0.00000022649232786295453, 0.0000000000000000002168404344971009,
     15, 2, 3, 6, 128, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_7_KS_PBS", 1018, 1004, 1, 32768, 0.00000005845871624688967, 0.0000000000000000002168404344971009,
     11, 3, 3, 7, 2, 128, "Big"),
    ("PARAM_MESSAGE_2_CARRY_6_KS_PBS", 1033, 987, 1, 32768, 0.00000007979529246348835, 0.0000000000000000002168404344971009,
     11, 3, 3, 7, 4, 64, "Big"),
    ("PARAM_MESSAGE_3_CARRY_5_KS_PBS", 1048, 985, 1, 32768, 0.00000008277032914509569, 0.0000000000000000002168404344971009,
     11, 3, 3, 7, 8, 32, "Big"),
    ("PARAM_MESSAGE_4_CARRY_4_KS_PBS", 1063, 996, 1, 32768, 0.00000006767666038309478, 0.0000000000000000002168404344971009,
     15, 2, 3, 7, 16, 16, "Big"),
    ("PARAM_MESSAGE_5_CARRY_3_KS_PBS", 1078, 1020, 1, 32768, 0.000000043618425315728666, 0.0000000000000000002168404344971009,
     15, 2, 4, 5, 32, 8, "Big"),
    ("PARAM_MESSAGE_6_CARRY_2_KS_PBS", 1093, 1018, 1, 32768, 0.000000045244666805696514, 0.0000000000000000002168404344971009,
     15, 2, 4, 5, 64, 4, "Big"),
    ("PARAM_MESSAGE_7_CARRY_1_KS_PBS", 1108, 1017, 1, 32768, 0.0000000460803851108693, 0.0000000000000000002168404344971009,
     15, 2, 4, 5, 128, 2, "Big"),
    ("PARAM_MESSAGE_8_CARRY_0_KS_PBS", 1123, 1017, 1, 32768, 0.0000000460803851108693, 0.0000000000000000002168404344971009,
     15, 2, 4, 5, 256, 1, "Big"),
    ("PARAM_MESSAGE_1_CARRY_1_PBS_KS", 1139, 783, 3, 512, 0.0000033382067621812462, 0.0000000000034525330484572114,
     18, 1, 5, 3, 2, 2, "Small"),
    ("PARAM_MESSAGE_2_CARRY_2_PBS_KS", 1155, 870, 1, 2048, 0.0000006791658447437413, 0.00000000000000029403601535432533,
     23, 1, 4, 4, 4, 4, "Small"),
    ("PARAM_MESSAGE_3_CARRY_3_PBS_KS", 1171, 1025, 1, 8192, 0.00000003980397588319241, 0.0000000000000000002168404344971009,
     15, 2, 4, 5, 8, 8, "Small"),
    ("PARAM_MESSAGE_4_CARRY_4_PBS_KS", 1187, 1214, 1, 32768, 0.0000000012520482863081104, 0.0000000000000000002168404344971009,
     15, 2, 4, 6, 16, 16, "Small"),
]

SHORTINT_ALL = {
    t[0]: ClassicPBSParameters(lwe_dimension=t[2], glwe_dimension=t[3], polynomial_size=t[4], lwe_modular_std_dev=t[5],
                               glwe_modular_std_dev=t[6], pbs_base_log=t[7], pbs_level=t[8], ks_base_log=t[9],
                               ks_level=t[10], message_modulus=t[11], carry_modulus=t[12], encryption_key_choice=t[13],
                               name=t[0])
    for t in _SHORTINT_TABLE}
SHORTINT_SOURCE_LINE = {t[0]: t[1] for t in _SHORTINT_TABLE}
assert SHORTINT_ALL["PARAM_MESSAGE_2_CARRY_2_KS_PBS"] == PARAM_MESSAGE_2_CARRY_2_KS_PBS
assert SHORTINT_ALL["PARAM_MESSAGE_4_CARRY_4_KS_PBS"] == PARAM_MESSAGE_4_CARRY_4_KS_PBS
globals().update(SHORTINT_ALL)

ALL = {p.name: p for p in [PARAM_MESSAGE_2_CARRY_2_KS_PBS, PARAM_MESSAGE_4_CARRY_4_KS_PBS,
                           PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS,
                           PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS, MANTICORE_PARAMETERS] + GADGET_ALL}
ALL.update(SHORTINT_ALL)
ALL.update(MULTI_BIT_ALL)


# The compact-public-key sets (shortint/parameters/parameters_compact_pk.rs:13-70, all 56): the dimension of the
# encryption key (k N for KS_PBS, n for PBS_KS) is a power of two, as a CompactPublicKey needs.  Same columns as
# _SHORTINT_TABLE.  Kept apart from ALL: COMPACT_PK_ALL holds the sets the engine accepts (context creation
# succeeds and an existing keyswitch arm takes the keyswitch decomposition), COMPACT_PK_REFUSED names every other
# one with the engine's refusal.
_COMPACT_PK_TABLE = [
    ("PARAM_MESSAGE_1_CARRY_1_COMPACT_PK_KS_PBS", 71, 638, 1, 1024, 6.150656787521441e-05, 4.9902938117294516e-08,
     6, 3, 2, 6, 2, 2, "Big"),
    ("PARAM_MESSAGE_1_CARRY_2_COMPACT_PK_KS_PBS", 86, 710, 1, 2048, 1.6307554775887557e-05, 3.152834667799722e-16,
     21, 1, 3, 4, 2, 4, "Big"),
    ("PARAM_MESSAGE_1_CARRY_3_COMPACT_PK_KS_PBS", 101, 756, 1, 2048, 6.983104533665408e-06, 3.152834667799722e-16,
     21, 1, 3, 5, 2, 8, "Big"),
    ("PARAM_MESSAGE_1_CARRY_4_COMPACT_PK_KS_PBS", 116, 821, 1, 4096, 2.1066761751849058e-06, 2.168404344971009e-19,
     22, 1, 3, 5, 2, 16, "Big"),
    ("PARAM_MESSAGE_1_CARRY_5_COMPACT_PK_KS_PBS", 131, 888, 1, 8192, 6.12494404462554e-07, 2.168404344971009e-19,
     22, 1, 3, 6, 2, 32, "Big"),
    ("PARAM_MESSAGE_1_CARRY_6_COMPACT_PK_KS_PBS", 146, 942, 1, 16384, 2.2630942423569665e-07, 2.168404344971009e-19,
     14, 2, 3, 6, 2, 64, "Big"),
    ("PARAM_MESSAGE_1_CARRY_7_COMPACT_PK_KS_PBS", 161, 1029, 1, 32768, 4.5508144326041556e-08, 2.168404344971009e-19,
     14, 2, 4, 5, 2, 128, "Big"),
    ("PARAM_MESSAGE_2_CARRY_1_COMPACT_PK_KS_PBS", 176, 710, 1, 2048, 1.6307554775887557e-05, 3.152834667799722e-16,
     22, 1, 3, 4, 4, 2, "Big"),
    ("PARAM_MESSAGE_2_CARRY_2_COMPACT_PK_KS_PBS", 191, 756, 1, 2048, 6.983104533665408e-06, 3.152834667799722e-16,
     22, 1, 3, 5, 4, 4, "Big"),
    ("PARAM_MESSAGE_2_CARRY_3_COMPACT_PK_KS_PBS", 206, 850, 1, 4096, 1.2341934723690542e-06, 2.168404344971009e-19,
     22, 1, 4, 4, 4, 8, "Big"),
    ("PARAM_MESSAGE_2_CARRY_4_COMPACT_PK_KS_PBS", 221, 877, 1, 8192, 7.502111286917793e-07, 2.168404344971009e-19,
     14, 2, 3, 6, 4, 16, "Big"),
    ("PARAM_MESSAGE_2_CARRY_5_COMPACT_PK_KS_PBS", 236, 942, 1, 16384, 2.2630942423569665e-07, 2.168404344971009e-19,
     14, 2, 3, 6, 4, 32, "Big"),
    ("PARAM_MESSAGE_2_CARRY_6_COMPACT_PK_KS_PBS", 251, 1030, 1, 32768, 4.46767660406645e-08, 2.168404344971009e-19,
     14, 2, 4, 5, 4, 64, "Big"),
    ("PARAM_MESSAGE_3_CARRY_1_COMPACT_PK_KS_PBS", 266, 759, 1, 2048, 6.607793351104514e-06, 3.152834667799722e-16,
     23, 1, 3, 5, 8, 2, "Big"),
    ("PARAM_MESSAGE_3_CARRY_2_COMPACT_PK_KS_PBS", 281, 862, 1, 4096, 9.892236038140916e-07, 2.168404344971009e-19,
     22, 1, 3, 6, 8, 4, "Big"),
    ("PARAM_MESSAGE_3_CARRY_3_COMPACT_PK_KS_PBS", 296, 877, 1, 8192, 7.502111286917793e-07, 2.168404344971009e-19,
     14, 2, 3, 6, 8, 8, "Big"),
    ("PARAM_MESSAGE_3_CARRY_4_COMPACT_PK_KS_PBS", 311, 942, 1, 16384, 2.2630942423569665e-07, 2.168404344971009e-19,
     14, 2, 3, 6, 8, 16, "Big"),
    ("PARAM_MESSAGE_3_CARRY_5_COMPACT_PK_KS_PBS", 326, 1032, 1, 32768, 4.305929680023812e-08, 2.168404344971009e-19,
     14, 2, 4, 5, 8, 32, "Big"),
    ("PARAM_MESSAGE_4_CARRY_1_COMPACT_PK_KS_PBS", 341, 820, 1, 4096, 2.145878762605306e-06, 2.168404344971009e-19,
     14, 2, 3, 5, 16, 2, "Big"),
    ("PARAM_MESSAGE_4_CARRY_2_COMPACT_PK_KS_PBS", 356, 877, 1, 8192, 7.502111286917793e-07, 2.168404344971009e-19,
     14, 2, 3, 6, 16, 4, "Big"),
    ("PARAM_MESSAGE_4_CARRY_3_COMPACT_PK_KS_PBS", 371, 943, 1, 16384, 2.2219042764335445e-07, 2.168404344971009e-19,
     15, 2, 3, 6, 16, 8, "Big"),
    ("PARAM_MESSAGE_4_CARRY_4_COMPACT_PK_KS_PBS", 386, 1044, 1, 32768, 3.4512638181977925e-08, 2.168404344971009e-19,
     15, 2, 4, 5, 16, 16, "Big"),
    ("PARAM_MESSAGE_5_CARRY_1_COMPACT_PK_KS_PBS", 401, 877, 1, 8192, 7.502111286917793e-07, 2.168404344971009e-19,
     15, 2, 3, 6, 32, 2, "Big"),
    ("PARAM_MESSAGE_5_CARRY_2_COMPACT_PK_KS_PBS", 416, 947, 1, 16384, 2.0639337523302752e-07, 2.168404344971009e-19,
     15, 2, 3, 6, 32, 4, "Big"),
    ("PARAM_MESSAGE_5_CARRY_3_COMPACT_PK_KS_PBS", 431, 997, 1, 32768, 8.20967300015962e-08, 2.168404344971009e-19,
     11, 3, 3, 7, 32, 8, "Big"),
    ("PARAM_MESSAGE_6_CARRY_1_COMPACT_PK_KS_PBS", 446, 942, 1, 16384, 2.2630942423569665e-07, 2.168404344971009e-19,
     11, 3, 3, 6, 64, 2, "Big"),
    ("PARAM_MESSAGE_6_CARRY_2_COMPACT_PK_KS_PBS", 461, 998, 1, 32768, 8.05969228871865e-08, 2.168404344971009e-19,
     11, 3, 3, 7, 64, 4, "Big"),
    ("PARAM_MESSAGE_7_CARRY_1_COMPACT_PK_KS_PBS", 476, 1017, 1, 32768, 5.6777713805325606e-08, 2.168404344971009e-19,
     11, 3, 3, 7, 128, 2, "Big"),
    ("PARAM_MESSAGE_1_CARRY_1_COMPACT_PK_PBS_KS", 493, 1024, 3, 512, 4.99029381172945e-08, 3.9666940817241e-12,
     18, 1, 8, 2, 2, 2, "Small"),
    ("PARAM_MESSAGE_1_CARRY_2_COMPACT_PK_PBS_KS", 508, 1024, 2, 1024, 4.99029381172945e-08, 3.15283466779972e-16,
     18, 1, 8, 2, 2, 4, "Small"),
    ("PARAM_MESSAGE_1_CARRY_3_COMPACT_PK_PBS_KS", 523, 1024, 1, 2048, 4.99029381172945e-08, 3.15283466779972e-16,
     21, 1, 8, 2, 2, 8, "Small"),
    ("PARAM_MESSAGE_1_CARRY_4_COMPACT_PK_PBS_KS", 538, 1024, 1, 4096, 4.99029381172945e-08, 2.16840434497101e-19,
     21, 1, 6, 3, 2, 16, "Small"),
    ("PARAM_MESSAGE_1_CARRY_5_COMPACT_PK_PBS_KS", 553, 1024, 1, 8192, 4.99029381172945e-08, 2.16840434497101e-19,
     22, 1, 5, 4, 2, 32, "Small"),
    ("PARAM_MESSAGE_1_CARRY_6_COMPACT_PK_PBS_KS", 568, 1024, 1, 16384, 4.99029381172945e-08, 2.16840434497101e-19,
     12, 2, 4, 5, 2, 64, "Small"),
    ("PARAM_MESSAGE_1_CARRY_7_COMPACT_PK_PBS_KS", 583, 1024, 1, 32768, 4.99029381172945e-08, 2.16840434497101e-19,
     14, 2, 2, 11, 2, 128, "Small"),
    ("PARAM_MESSAGE_2_CARRY_1_COMPACT_PK_PBS_KS", 598, 1024, 2, 1024, 4.99029381172945e-08, 3.15283466779972e-16,
     21, 1, 8, 2, 4, 2, "Small"),
    ("PARAM_MESSAGE_2_CARRY_2_COMPACT_PK_PBS_KS", 613, 1024, 1, 2048, 4.99029381172945e-08, 3.15283466779972e-16,
     21, 1, 8, 2, 4, 4, "Small"),
    ("PARAM_MESSAGE_2_CARRY_3_COMPACT_PK_PBS_KS", 628, 1024, 1, 4096, 4.99029381172945e-08, 2.16840434497101e-19,
     21, 1, 6, 3, 4, 8, "Small"),
    ("PARAM_MESSAGE_2_CARRY_4_COMPACT_PK_PBS_KS", 643, 1024, 1, 8192, 4.99029381172945e-08, 2.16840434497101e-19,
     12, 2, 5, 4, 4, 16, "Small"),
    ("PARAM_MESSAGE_2_CARRY_5_COMPACT_PK_PBS_KS", 658, 1024, 1, 16384, 4.99029381172945e-08, 2.16840434497101e-19,
     14, 2, 3, 7, 4, 32, "Small"),
    ("PARAM_MESSAGE_2_CARRY_6_COMPACT_PK_PBS_KS", 673, 2048, 1, 65536, 3.15283466779972e-16, 2.16840434497101e-19,
     14, 2, 25, 1, 4, 64, "Small"),
    ("PARAM_MESSAGE_3_CARRY_1_COMPACT_PK_PBS_KS", 688, 1024, 1, 2048, 4.99029381172945e-08, 3.15283466779972e-16,
     22, 1, 6, 3, 8, 2, "Small"),
    ("PARAM_MESSAGE_3_CARRY_2_COMPACT_PK_PBS_KS", 703, 1024, 1, 4096, 4.99029381172945e-08, 2.16840434497101e-19,
     12, 2, 5, 4, 8, 4, "Small"),
    ("PARAM_MESSAGE_3_CARRY_3_COMPACT_PK_PBS_KS", 718, 1024, 1, 8192, 4.99029381172945e-08, 2.16840434497101e-19,
     12, 2, 3, 7, 8, 8, "Small"),
    ("PARAM_MESSAGE_3_CARRY_4_COMPACT_PK_PBS_KS", 733, 1024, 1, 16384, 4.99029381172945e-08, 2.16840434497101e-19,
     14, 2, 1, 22, 8, 16, "Small"),
    ("PARAM_MESSAGE_3_CARRY_5_COMPACT_PK_PBS_KS", 748, 2048, 1, 65536, 3.15283466779972e-16, 2.16840434497101e-19,
     14, 2, 25, 1, 8, 32, "Small"),
    ("PARAM_MESSAGE_4_CARRY_1_COMPACT_PK_PBS_KS", 763, 1024, 1, 4096, 4.99029381172945e-08, 2.16840434497101e-19,
     12, 2, 2, 11, 16, 2, "Small"),
    ("PARAM_MESSAGE_4_CARRY_2_COMPACT_PK_PBS_KS", 778, 1024, 1, 8192, 4.99029381172945e-08, 2.16840434497101e-19,
     9, 3, 1, 21, 16, 4, "Small"),
    ("PARAM_MESSAGE_4_CARRY_3_COMPACT_PK_PBS_KS", 793, 2048, 1, 32768, 3.15283466779972e-16, 2.16840434497101e-19,
     14, 2, 25, 1, 16, 8, "Small"),
    ("PARAM_MESSAGE_4_CARRY_4_COMPACT_PK_PBS_KS", 808, 2048, 1, 65536, 3.15283466779972e-16, 2.16840434497101e-19,
     11, 3, 25, 1, 16, 16, "Small"),
    ("PARAM_MESSAGE_5_CARRY_1_COMPACT_PK_PBS_KS", 823, 2048, 1, 16384, 3.15283466779972e-16, 2.16840434497101e-19,
     14, 2, 25, 1, 32, 2, "Small"),
    ("PARAM_MESSAGE_5_CARRY_2_COMPACT_PK_PBS_KS", 838, 2048, 1, 32768, 3.15283466779972e-16, 2.16840434497101e-19,
     14, 2, 25, 1, 32, 4, "Small"),
    ("PARAM_MESSAGE_5_CARRY_3_COMPACT_PK_PBS_KS", 853, 2048, 1, 65536, 3.15283466779972e-16, 2.16840434497101e-19,
     11, 3, 25, 1, 32, 8, "Small"),
    ("PARAM_MESSAGE_6_CARRY_1_COMPACT_PK_PBS_KS", 868, 2048, 1, 32768, 3.15283466779972e-16, 2.16840434497101e-19,
     11, 3, 25, 1, 64, 2, "Small"),
    ("PARAM_MESSAGE_6_CARRY_2_COMPACT_PK_PBS_KS", 883, 2048, 1, 65536, 3.15283466779972e-16, 2.16840434497101e-19,
     11, 3, 17, 2, 64, 4, "Small"),
    ("PARAM_MESSAGE_7_CARRY_1_COMPACT_PK_PBS_KS", 898, 2048, 1, 65536, 3.15283466779972e-16, 2.16840434497101e-19,
     9, 4, 17, 2, 128, 2, "Small"),
]

# (name, the engine's refusal): context creation finds no PBS kernel at N = 65536; the context's keyswitch fails its
# launch for ks_base_log > 7 (8 x 2, 17 x 2, 25 x 1: its int8-MFMA and int8 scalar arms hold digits of at most 7 bits;
# the 16-bit-digit scalar form serves key objects only)
COMPACT_PK_REFUSED = (
    ("PARAM_MESSAGE_1_CARRY_1_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_1_CARRY_2_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_1_CARRY_3_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_2_CARRY_1_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_2_CARRY_2_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_2_CARRY_6_COMPACT_PK_PBS_KS", "no kernel for N=65536 k=1 pbs_level=2"),
    ("PARAM_MESSAGE_3_CARRY_5_COMPACT_PK_PBS_KS", "no kernel for N=65536 k=1 pbs_level=2"),
    ("PARAM_MESSAGE_4_CARRY_3_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_4_CARRY_4_COMPACT_PK_PBS_KS", "no kernel for N=65536 k=1 pbs_level=3"),
    ("PARAM_MESSAGE_5_CARRY_1_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_5_CARRY_2_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_5_CARRY_3_COMPACT_PK_PBS_KS", "no kernel for N=65536 k=1 pbs_level=3"),
    ("PARAM_MESSAGE_6_CARRY_1_COMPACT_PK_PBS_KS", "launch keyswitch: invalid argument"),
    ("PARAM_MESSAGE_6_CARRY_2_COMPACT_PK_PBS_KS", "no kernel for N=65536 k=1 pbs_level=3"),
    ("PARAM_MESSAGE_7_CARRY_1_COMPACT_PK_PBS_KS", "no kernel for N=65536 k=1 pbs_level=4"),
)
COMPACT_PK_NAMES = tuple(t[0] for t in _COMPACT_PK_TABLE)
COMPACT_PK_ALL = {
    t[0]: ClassicPBSParameters(lwe_dimension=t[2], glwe_dimension=t[3], polynomial_size=t[4], lwe_modular_std_dev=t[5],
                               glwe_modular_std_dev=t[6], pbs_base_log=t[7], pbs_level=t[8], ks_base_log=t[9],
                               ks_level=t[10], message_modulus=t[11], carry_modulus=t[12], encryption_key_choice=t[13],
                               name=t[0])
    for t in _COMPACT_PK_TABLE if t[0] not in dict(COMPACT_PK_REFUSED)}
COMPACT_PK_SOURCE_LINE = {t[0]: t[1] for t in _COMPACT_PK_TABLE}
globals().update(COMPACT_PK_ALL)


@dataclass(frozen=True)
class WopbsParameters(ClassicPBSParameters):
    """Mirror of shortint WopbsParameters (shortint/parameters/mod.rs): the classic fields plus the
    private functional packing keyswitch and circuit bootstrap decompositions.  Usable wherever a
    ClassicPBSParameters creates a context."""

    pfks_base_log: int = 0
    pfks_level: int = 0
    pfks_modular_std_dev: float = 0.0
    cbs_base_log: int = 0
    cbs_level: int = 0


# shortint/parameters/parameters_wopbs_message_carry.rs:272-291, 292-311, 432-451
WOPBS_PARAM_MESSAGE_1_CARRY_1_KS_PBS = WopbsParameters(
    lwe_dimension=653, glwe_dimension=1, polynomial_size=2048,
    lwe_modular_std_dev=0.00003604499526942373, glwe_modular_std_dev=0.00000000000000029403601535432533,
    pbs_base_log=15, pbs_level=2, ks_base_log=5, ks_level=2, message_modulus=2, carry_modulus=2,
    pfks_base_log=15, pfks_level=2, pfks_modular_std_dev=0.00000000000000029403601535432533,
    cbs_base_log=5, cbs_level=3, name="WOPBS_PARAM_MESSAGE_1_CARRY_1_KS_PBS")
WOPBS_PARAM_MESSAGE_1_CARRY_2_KS_PBS = WopbsParameters(
    lwe_dimension=487, glwe_dimension=3, polynomial_size=512,
    lwe_modular_std_dev=0.00054842163045222410337, glwe_modular_std_dev=0.000000000002573000821792597679153983627,
    pbs_base_log=9, pbs_level=3, ks_base_log=2, ks_level=4, message_modulus=2, carry_modulus=4,
    pfks_base_log=9, pfks_level=3, pfks_modular_std_dev=0.000000000002573000821792597679153983627,
    cbs_base_log=3, cbs_level=5, name="WOPBS_PARAM_MESSAGE_1_CARRY_2_KS_PBS")
WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS = WopbsParameters(
    lwe_dimension=769, glwe_dimension=1, polynomial_size=2048,
    lwe_modular_std_dev=0.0000043131554647504185, glwe_modular_std_dev=0.00000000000000029403601535432533,
    pbs_base_log=15, pbs_level=2, ks_base_log=6, ks_level=2, message_modulus=4, carry_modulus=4,
    pfks_base_log=15, pfks_level=2, pfks_modular_std_dev=0.00000000000000029403601535432533,
    cbs_base_log=5, cbs_level=3, name="WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS")
WOPBS_ALL = {p.name: p for p in [WOPBS_PARAM_MESSAGE_1_CARRY_1_KS_PBS, WOPBS_PARAM_MESSAGE_1_CARRY_2_KS_PBS,
                                 WOPBS_PARAM_MESSAGE_2_CARRY_2_KS_PBS]}


# ---- boolean module (32-bit torus) -----------------------------------------------------------------
@dataclass(frozen=True)
class BooleanParameters:
    """Mirror of BooleanParameters (boolean/parameters/mod.rs:34-64).  The ciphertext words are u32;
    encryption_key_choice "Small" = PBSOrder::BootstrapKeyswitch, "Big" = PBSOrder::KeyswitchBootstrap."""

    lwe_dimension: int
    glwe_dimension: int
    polynomial_size: int
    lwe_modular_std_dev: float
    glwe_modular_std_dev: float
    pbs_base_log: int
    pbs_level: int
    ks_base_log: int
    ks_level: int
    encryption_key_choice: str
    name: str = ""
    # fields the engine's context reads from every parameter set; the 32-bit calls ignore the moduli
    message_modulus: int = 2
    carry_modulus: int = 1
    grouping_factor: int = 0

    @property
    def big_lwe_dimension(self) -> int:
        return self.glwe_dimension * self.polynomial_size

    @property
    def pbs_order(self) -> int:
        """1 = BootstrapKeyswitch (ciphertexts under the small key), 0 = KeyswitchBootstrap."""
        return 1 if self.encryption_key_choice == "Small" else 0

    @property
    def ciphertext_words(self) -> int:
        return (self.lwe_dimension if self.pbs_order else self.big_lwe_dimension) + 1


BOOLEAN_DEFAULT_PARAMETERS = BooleanParameters(
    lwe_dimension=722, glwe_dimension=2, polynomial_size=512,
    lwe_modular_std_dev=0.000013071021089943935, glwe_modular_std_dev=0.00000004990272175010415,
    pbs_base_log=6, pbs_level=3, ks_base_log=3, ks_level=4,
    encryption_key_choice="Small", name="DEFAULT_PARAMETERS")
BOOLEAN_DEFAULT_PARAMETERS_KS_PBS = BooleanParameters(
    lwe_dimension=664, glwe_dimension=2, polynomial_size=512,
    lwe_modular_std_dev=0.00003808282923459771, glwe_modular_std_dev=0.00000004990272175010415,
    pbs_base_log=6, pbs_level=3, ks_base_log=3, ks_level=4,
    encryption_key_choice="Big", name="DEFAULT_PARAMETERS_KS_PBS")
BOOLEAN_PARAMETERS_ERROR_PROB_2_POW_MINUS_165 = BooleanParameters(
    lwe_dimension=767, glwe_dimension=2, polynomial_size=1024,
    lwe_modular_std_dev=0.000005104350373791501, glwe_modular_std_dev=0.0000000009313225746154785,
    pbs_base_log=10, pbs_level=2, ks_base_log=3, ks_level=5,
    encryption_key_choice="Small", name="PARAMETERS_ERROR_PROB_2_POW_MINUS_165")
BOOLEAN_PARAMETERS_ERROR_PROB_2_POW_MINUS_165_KS_PBS = BooleanParameters(
    lwe_dimension=700, glwe_dimension=1, polynomial_size=1024,
    lwe_modular_std_dev=0.0000196095987892077, glwe_modular_std_dev=0.00000004990272175010415,
    pbs_base_log=5, pbs_level=4, ks_base_log=2, ks_level=7,
    encryption_key_choice="Big", name="PARAMETERS_ERROR_PROB_2_POW_MINUS_165_KS_PBS")
BOOLEAN_TFHE_LIB_PARAMETERS = BooleanParameters(
    lwe_dimension=630, glwe_dimension=1, polynomial_size=1024,
    lwe_modular_std_dev=0.000030517578125, glwe_modular_std_dev=0.00000002980232238769531,
    pbs_base_log=7, pbs_level=3, ks_base_log=2, ks_level=8,
    encryption_key_choice="Small", name="TFHE_LIB_PARAMETERS")
BOOLEAN_PARAMETER_SETS = (
    BOOLEAN_DEFAULT_PARAMETERS, BOOLEAN_DEFAULT_PARAMETERS_KS_PBS, BOOLEAN_PARAMETERS_ERROR_PROB_2_POW_MINUS_165,
    BOOLEAN_PARAMETERS_ERROR_PROB_2_POW_MINUS_165_KS_PBS, BOOLEAN_TFHE_LIB_PARAMETERS)
