"""Batched integer radix layer on top of the GPU PBS engine.

Mirror of the reference's radix_parallel multiplication DAG, executed for K independent
operand pairs at once:

  ServerKey.mul_parallelized / mul_assign_parallelized      integer/server_key/radix_parallel/mul.rs:553-590
  ServerKey.unchecked_mul_assign_parallelized               mul.rs:300-414
  ServerKey.unchecked_sum_ciphertexts_vec_parallelized      radix_parallel/add.rs:783-960
  ServerKey.add_assign_parallelized                         add.rs:206-242
  unchecked_add_assign_parallelized_low_latency,
  propagate_single_carry_parallelized_low_latency,
  compute_carry_propagation_parallelized_low_latency,
  compute_prefix_sum_hillis_steele, generate_init_carry_array
                                                            add.rs:487-771
  full_propagate_parallelized / partial_propagate_parallelized
                                                            radix_parallel/mod.rs:88-155
  ServerKey.blockshift                                      radix/scalar_mul.rs:345-355
  ServerKey neg, sub, bitand / bitor / bitxor / bitnot, eq / ne, gt / ge / lt / le, if_then_else / cmux, min / max
  (unchecked and default forms, unsigned)                   radix/neg.rs, radix_parallel/{neg,sub,bitwise_op,comparison,
                                                            cmux}.rs, comparator.rs: see "neg, sub, ..." in ServerKey
  ServerKey scalar_{left_shift,right_shift,rotate_left,rotate_right}, {left_shift,right_shift,rotate_left,
  rotate_right} by an encrypted amount (barrel_shifter), scalar_mul (unchecked and default forms, unsigned)
                                                            radix_parallel/{scalar_shift,scalar_rotate,shift,rotate,
                                                            bit_extractor,scalar_mul}.rs
  ServerKey scalar_add, scalar_sub, scalar_bit{and,or,xor}, scalar_{eq,ne,gt,ge,lt,le,max,min} (unchecked and default
  forms, unsigned; one clear operand per batch or per row)
                                                            radix/scalar_{add,sub}.rs, radix_parallel/scalar_{add,sub,
                                                            bitwise_op,comparison}.rs, comparator.rs: see "clear
                                                            operands" in ServerKey
  ServerKey unsigned_overflowing_sub, div_rem, div, rem (unchecked and default forms, unsigned), the zero tests
  compare_blocks_with_zero, is_at_least_one_comparisons_block_true, are_all_comparisons_block_true
                                                            radix_parallel/{sub,div_mod,scalar_comparison}.rs,
                                                            shortint/server_key/{sub,neg}.rs: see "overflowing
                                                            sub, zero tests, division" in ServerKey
  shortint generate_lookup_table_bivariate_with_factor      shortint/server_key/bivariate_pbs.rs:71-96
  shortint unchecked_apply_lookup_table_bivariate_assign    shortint/server_key/bivariate_pbs.rs:69-182
  WopbsKey (wopbs, wopbs_without_padding, bivariate_wopbs_with_degree, generate_lut_radix,
  generate_lut_radix_without_padding, generate_lut_bivariate_radix, keyswitch_to_wopbs_params,
  keyswitch_to_pbs_params), encode_radix, encode_mix_radix, decode_radix,
  split_value_according_to_bit_basis                        integer/wopbs/mod.rs:94-195, 216-629, 784-844

Execution model.  The reference's DAG depends only on block degrees and noise levels, never on
the encrypted values, so K operand pairs with the same input shape follow the same DAG.  A
RadixBatch therefore stores the K ciphertexts as one u64 array [K, blocks, lwe_size] with a single
(degree, noise_level) per block, and every PBS layer of the DAG -- across all terms and all K
pairs -- is handed to the engine as ONE batched keyswitch+PBS launch with per-ciphertext LUT
indexes (the "PBS-DAG scheduler" of SURVEY.md 8f row f1).  Trivial blocks take the reference's
trivial-PBS shortcut (shortint/server_key/mod.rs:763-781).  With the GPU engine the batch stays
resident in HBM between layers (torch tensors for storage; the LWE arithmetic and trivial PBS in
the engine's lwe_ops kernels); with any other engine object (the oracle, in the tests) it is a
numpy array on the host -- same DAG, same bits.

Carry propagation uses the Hillis-Steele branch; the reference selects it whenever
should_hillis_steele_propagation_be_faster (add.rs:44-76) holds, i.e. with >= 16 rayon threads
for 16 blocks.  The reference's sequential branch is not implemented: on a modulus pair the Hillis-Steele
branch and the chunked sum cannot serve (propagation_refusal, mul_refusal) the carry-propagating entry
points raise NotImplementedError before any PBS.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .shortint import (KEYSWITCH_BOOTSTRAP, NOISE_NOMINAL, NOISE_ZERO, LookupTable, ServerKey as ShortintServerKey,
                       WopbsKey as ShortintWopbsKey)

OUTPUT_CARRY_NONE, OUTPUT_CARRY_GENERATED, OUTPUT_CARRY_PROPAGATED = 0, 1, 2  # add.rs:13-21


@dataclass
class RadixBatch:
    """K radix ciphertexts with shared block metadata (integer/ciphertext/mod.rs RadixCiphertext)."""

    data: np.ndarray      # [K, blocks, lwe_size] u64
    degree: list          # per block
    noise: list           # per block

    @property
    def count(self) -> int:
        return self.data.shape[0]

    @property
    def num_blocks(self) -> int:
        return self.data.shape[1]

    def clone(self) -> "RadixBatch":
        d = self.data.copy() if isinstance(self.data, np.ndarray) else self.data.clone()
        return RadixBatch(d, list(self.degree), list(self.noise))

    def block_carries_are_empty(self, message_modulus: int) -> bool:
        return all(d < message_modulus for d in self.degree)

    def holds_boolean_value(self) -> bool:
        return self.degree[0] <= 1 and all(d == 0 for d in self.degree[1:])

    def is_trivial_block(self, j: int) -> bool:
        return self.noise[j] == NOISE_ZERO


class _LutFamily:
    """The LUTs a clear digit chooses from: row r of a request takes luts[digit(r)].  One object per family for the
    life of the key, as for a LookupTable (the device caches go by identity)."""

    def __init__(self, luts):
        self.luts = list(luts)
        self.degree = max(lut.degree for lut in self.luts)


class _ClearRows:
    """One clear operand per row of a batch, as u64: a numpy uint64 array on the host (uploaded once per call on
    the device path) or a torch int64 tensor on the engine's device (read in place: nothing is copied or checked)."""

    def __init__(self, host=None, dev=None):
        self.host, self.dev = host, dev

    def on_host(self) -> np.ndarray:
        if self.host is None:
            self.host = self.dev.cpu().numpy().view(np.uint64)
        return self.host

    def on_device(self, ops):
        if self.dev is None:
            self.dev = ops.from_host(self.host)
        return self.dev


class _PbsLayer:
    """Collects the independent LUT applications of one DAG layer and runs them in one launch.

    A request may carry a prepare op: the PBS input is then not block j of the batch as it stands but
        sum over terms of scalar * block i of a source batch  +  body_add on the body,
    the packing, subtraction or sum the reference does on the block right before the LUT, and the PBS output
    lands in block j with post_add * delta added to its body (compare_block_assign's + 1).  A layer with such a
    request runs fused (flush_fused): ONE block-layer call assembles the input rows of every request in the
    layer's input buffer, the batched KS+PBS follows, ONE more block-layer call scatters the outputs to their
    blocks.  Layers without one keep the launch path below, as the multiply DAG pins it.

    A request may also carry a clear part: one clear operand per row, read on the device (flush_clear).  Between
    two PBS layers a clear operand is a plaintext on the body of a block or the choice of a LUT out of a family,
    and the first block-layer call of the layer takes both from the operand of each row, so the DAG and the tables
    of the layer do not depend on the clear values."""

    def __init__(self, sk: "ServerKey"):
        self.sk = sk
        # (batch, block, lut), with a prepare op (batch, block, lut, body_add, terms, post_add), with a clear part
        # or a LUT family (..., post_add, clear)
        self.reqs = []

    def add(self, rb: RadixBatch, j: int, lut, prepare=None, post_add: int = 0, clear=None):
        """prepare: (body_add, [(source batch, block, scalar), ...]); None with post_add = 0: block j as it is.
        clear: (_ClearRows, negate, shift, bits, scale): row r of the request also gets digit(r) * scale on the body
        of its PBS input, digit(r) = ((negate ? -c_r : c_r) >> shift) & (2^bits - 1) of its clear operand c_r; and
        where `lut` is a _LutFamily, row r takes its LUT number digit(r)."""
        if clear is not None or isinstance(lut, _LutFamily):
            body_add, terms = prepare if prepare is not None else (0, [(rb, j, 1)])
            self.reqs.append((rb, j, lut, body_add, list(terms), post_add, clear))
        elif prepare is None and not post_add:
            self.reqs.append((rb, j, lut))
        else:
            body_add, terms = prepare if prepare is not None else (0, [(rb, j, 1)])
            self.reqs.append((rb, j, lut, body_add, list(terms), post_add))

    def flush_fused(self, reqs):
        """The layer with prepare ops.  Request q of the non-trivial ones owns rows [qK, (q+1)K) of the input
        buffer.  A request whose sources are all trivial (or that has none) is a trivial ciphertext: its op
        writes block j itself, the trivial PBS follows on the block and it stays NOISE_ZERO."""
        sk, ops = self.sk, self.sk.ops
        reqs = [r if len(r) == 6 else (r[0], r[1], r[2], 0, [(r[0], r[1], 1)], 0) for r in reqs]
        K, size, delta = reqs[0][0].count, sk.lwe_size, sk.p.delta
        todo, triv, luts, lut_of = [], [], [], {}
        for req in reqs:
            if all(src.is_trivial_block(i) for src, i, _ in req[4]):
                triv.append(req)
                continue
            if id(req[2]) not in lut_of:
                lut_of[id(req[2])] = len(luts)
                luts.append(req[2])
            todo.append(req)
        x = ops.rows(len(todo) * K, size) if todo else None
        pre = [(x[q * K:(q + 1) * K], body_add, [(ops.block(src, i), s) for src, i, s in terms])
               for q, (_, _, _, body_add, terms, _) in enumerate(todo)]
        pre += [(ops.block(rb, j), body_add, [(ops.block(src, i), s) for src, i, s in terms])
                for rb, j, _, body_add, terms, _ in triv]
        ops.block_layer(pre)
        post = []
        for rb, j, lut, _, _, post_add in triv:
            ops.trivial_pbs(rb, j, lut)
            if post_add:
                post.append((ops.block(rb, j), post_add * delta, [(ops.block(rb, j), 1)]))
        if todo:
            out = ops.pbs_buffer(x, K, [lut_of[id(r[2])] for r in todo], luts)
            sk.pbs_count += len(todo) * K
            sk.launches += 1
            post += [(ops.block(rb, j), post_add * delta, [(out[q * K:(q + 1) * K], 1)])
                     for q, (rb, j, _, _, _, post_add) in enumerate(todo)]
        if post:
            ops.block_layer(post)
        for rb, j, lut, _, _, post_add in reqs:
            rb.degree[j] = lut.degree + post_add
        for rb, j, _, _, _, _ in todo:
            rb.noise[j] = NOISE_NOMINAL
        for rb, j, _, _, _, _ in triv:
            rb.noise[j] = NOISE_ZERO

    def flush_clear(self, reqs):
        """The layer with clear parts or LUT families: flush_fused's three calls, the first one the block layer
        with a clear digit per row (ops.clear_block_layer).  The LUT stack of the layer holds every family whole,
        and a request's rows take lut_base + digit(r), written to the layer's index array by the same call that
        assembles the rows; a fixed-LUT request goes through with no clear bits (its rows take lut_base).  A layer
        whose stack is one LUT needs no index array.  A fixed LUT whose request has a digit on the body, in a layer
        with other LUTs, stands 2^bits times in the stack, since the one digit of an op serves body and index.
        Trivial sources: a fixed-LUT request keeps the trivial shortcut, its op writes block j itself, clear part
        included.  A family request goes through the batched PBS whatever its sources (the trivial PBS takes one
        LUT for all rows) and comes out NOISE_NOMINAL: the one deviation from the reference's bookkeeping."""
        sk, ops = self.sk, self.sk.ops
        full = []
        for r in reqs:
            if len(r) == 3:
                r = (r[0], r[1], r[2], 0, [(r[0], r[1], 1)], 0)
            full.append(r if len(r) == 7 else r + (None,))
        K, size, delta = full[0][0].count, sk.lwe_size, sk.p.delta
        todo, triv = [], []
        for req in full:
            fixed = not isinstance(req[2], _LutFamily)
            (triv if fixed and all(src.is_trivial_block(i) for src, i, _ in req[4]) else todo).append(req)
        multi = len({id(r[2]) for r in todo}) > 1 or any(isinstance(r[2], _LutFamily) for r in todo)
        copies = {}       # fixed LUTs with a digit on the body: how often they stand in a stack of several LUTs
        for _, _, lut, _, _, _, clear in todo:
            if multi and clear is not None and clear[3] and not isinstance(lut, _LutFamily):
                copies[id(lut)] = max(copies.get(id(lut), 1), 1 << clear[3])
        luts, base_of = [], {}
        for _, _, lut, _, _, _, clear in todo:
            if id(lut) in base_of:
                continue
            base_of[id(lut)] = len(luts)
            if isinstance(lut, _LutFamily):
                assert clear is not None and 1 << clear[3] <= len(lut.luts)
                luts += lut.luts
            else:
                luts += [lut] * copies.get(id(lut), 1)
        x = ops.rows(len(todo) * K, size) if todo else None
        idx = ops.index_rows(len(todo) * K) if todo and multi else None

        def part(clear, q=None, lut_base=0):
            rows, negate, shift, bits, scale = clear if clear is not None else (None, 0, 0, 0, 0)
            index = idx[q * K:(q + 1) * K] if q is not None and idx is not None else None
            return dict(rows=rows, negate=negate, shift=shift, bits=bits, scale=scale, index=index, lut_base=lut_base)

        pre = [(x[q * K:(q + 1) * K], body_add, [(ops.block(src, i), s) for src, i, s in terms],
                part(clear, q, base_of[id(lut)])) for q, (_, _, lut, body_add, terms, _, clear) in enumerate(todo)]
        pre += [(ops.block(rb, j), body_add, [(ops.block(src, i), s) for src, i, s in terms], part(clear))
                for rb, j, _, body_add, terms, _, clear in triv]
        ops.clear_block_layer(pre)
        post = []
        for rb, j, lut, _, _, post_add, _ in triv:
            ops.trivial_pbs(rb, j, lut)
            if post_add:
                post.append((ops.block(rb, j), post_add * delta, [(ops.block(rb, j), 1)]))
        if todo:
            out = ops.pbs_buffer_indexed(x, luts, idx)
            sk.pbs_count += len(todo) * K
            sk.launches += 1
            post += [(ops.block(rb, j), post_add * delta, [(out[q * K:(q + 1) * K], 1)])
                     for q, (rb, j, _, _, _, post_add, _) in enumerate(todo)]
        if post:
            ops.block_layer(post)
        for rb, j, lut, _, _, post_add, _ in full:
            rb.degree[j] = lut.degree + post_add
        for rb, j, *_ in todo:
            rb.noise[j] = NOISE_NOMINAL
        for rb, j, *_ in triv:
            rb.noise[j] = NOISE_ZERO

    def flush(self):
        reqs, self.reqs = self.reqs, []
        if not reqs:
            return
        if any(len(r) == 7 for r in reqs):
            return self.flush_clear(reqs)
        if any(len(r) == 6 for r in reqs):
            return self.flush_fused(reqs)
        sk = self.sk
        todo, luts, lut_of = [], [], {}
        for rb, j, lut in reqs:
            if rb.is_trivial_block(j):
                sk._trivial_pbs(rb, j, lut)
                continue
            if id(lut) not in lut_of:
                lut_of[id(lut)] = len(luts)
                luts.append(lut)
            todo.append((rb, j, lut_of[id(lut)]))
        if todo:
            n = sk.ops.pbs_rows([(rb, j, li) for rb, j, li in todo], luts)
            sk.pbs_count += n
            sk.launches += 1
            for rb, j, _ in todo:
                rb.noise[j] = NOISE_NOMINAL
        for rb, j, lut in reqs:
            rb.degree[j] = lut.degree



def _is_gpu_engine(engine) -> bool:
    """A single-device GPU engine: radix batches stay in its HBM between layers (_DeviceOps).  A
    multi-device context (Engine(devices=[...])) takes the host path instead: every layer is ONE
    host-pointer KS+PBS call, which the context splits over its devices -- the reference's one
    process with its rayon pool (radix_parallel/mul.rs:347-407) on the one-process drop-in."""
    from .engine import Engine

    return isinstance(engine, Engine) and not engine.multi_device


class _HostOps:
    """numpy arrays on the host; PBS through the engine's host-pointer API (any engine object
    with keyswitch_programmable_bootstrap, e.g. the oracle's in the tests)."""

    def __init__(self, sk: "ServerKey"):
        self.sk = sk

    def zeros(self, k, b, s):
        return np.zeros((k, b, s), dtype=np.uint64)

    def roll(self, data, shift):
        return np.roll(data, shift, axis=1)

    def to_host(self, data):
        return data

    def from_host(self, data):
        return data

    def copy_block(self, dst, j, src, i):
        dst.data[:, j, :] = src.data[:, i, :]

    def set_trivial(self, rb, j, body):
        rb.data[:, j, :] = 0
        rb.data[:, j, -1] = np.uint64(body)

    def mul_add(self, dst, j, scalar, src, i):
        if scalar != 1:
            dst.data[:, j, :] *= np.uint64(scalar)
        if src is not None:
            dst.data[:, j, :] += src.data[:, i, :]

    def trivial_pbs(self, rb, j, lut):
        p = self.sk.p
        modulus_sup = p.message_modulus * p.carry_modulus
        box = p.polynomial_size // modulus_sup
        body = lut.acc[p.glwe_dimension * p.polynomial_size:]
        value = rb.data[:, j, -1] // np.uint64(p.delta)
        neg = value >= np.uint64(modulus_sup)
        entry = body[((value % np.uint64(modulus_sup)) * np.uint64(box)).astype(np.int64)]
        rb.data[:, j, -1] = np.where(neg, np.uint64(0) - entry, entry)

    def rows(self, n, s):
        return np.empty((n, s), dtype=np.uint64)

    def block(self, rb, j):
        return rb.data[:, j, :]

    def block_layer(self, ops):
        """The block layer's formula, the reference of the device kernel (lwe_block_layer_kernel): for every
        op (dst, body_add, [(src, scalar), ...]) over [K, words] views,
            dst[r][w] = sum_t scalar_t * src_t[r][w] + (w == words - 1 ? body_add : 0)   wrapping mod 2^64.
        A source may be the destination itself; nothing else may overlap a destination."""
        for dst, body_add, terms in ops:
            acc = np.zeros(dst.shape, dtype=np.uint64)
            for src, scalar in terms:
                acc += np.uint64(scalar % (1 << 64)) * src
            acc[:, -1] += np.uint64(body_add % (1 << 64))
            dst[...] = acc

    def clear_block_layer(self, ops):
        """The block layer with a clear digit per row, the reference of the device kernel
        (lwe_clear_block_layer_kernel): block_layer's op with a fourth member, the dict flush_clear builds.  Row r:
            digit(r) = ((negate ? 0 - c_r : c_r) >> shift) & (2^bits - 1),   c_r = rows[r] (rows None: 0)
            dst[r][words - 1] += digit(r) * scale,   index[r] = lut_base + digit(r)   (index None: not written)."""
        for dst, body_add, terms, c in ops:
            acc = np.zeros(dst.shape, dtype=np.uint64)
            for src, scalar in terms:
                acc += np.uint64(scalar % (1 << 64)) * src
            digit = np.zeros(dst.shape[0], dtype=np.uint64)
            if c["rows"] is not None:
                v = c["rows"].on_host()
                v = (np.uint64(0) - v) if c["negate"] else v
                digit = (v >> np.uint64(c["shift"])) & np.uint64((1 << c["bits"]) - 1)
            acc[:, -1] += np.uint64(body_add % (1 << 64)) + digit * np.uint64(c["scale"] % (1 << 64))
            dst[...] = acc
            if c["index"] is not None:
                c["index"][...] = (np.uint64(c["lut_base"]) + digit).astype(np.uint32)

    def index_rows(self, n):
        return np.empty(n, dtype=np.uint32)

    def pbs_buffer(self, x, K, lut_of_request, luts):
        idx = np.repeat(np.asarray(lut_of_request, dtype=np.uint32), K)
        return self.sk.shortint.engine_ks_pbs(x, np.stack([lut.acc for lut in luts]), idx if len(luts) > 1 else None)

    def pbs_buffer_indexed(self, x, luts, idx):
        """batched KS+PBS of the rows of x, row r with LUT idx[r] of `luts` (idx None: the one LUT)"""
        return self.sk.shortint.engine_ks_pbs(x, np.stack([lut.acc for lut in luts]), idx)

    def plan(self, key, luts):
        """nothing to keep on the host: every layer hands its LUTs to the engine"""
        from contextlib import nullcontext

        return nullcontext()

    def pbs_rows(self, todo, luts):
        K = todo[0][0].count
        x = np.concatenate([rb.data[:, j, :] for rb, j, _ in todo], axis=0)
        idx = np.repeat(np.asarray([li for _, _, li in todo], dtype=np.uint32), K)
        out = self.sk.shortint.engine_ks_pbs(x, np.stack([lut.acc for lut in luts]), idx if len(luts) > 1 else None)
        for q, (rb, j, _) in enumerate(todo):
            rb.data[:, j, :] = out[q * K:(q + 1) * K]
        return x.shape[0]


class _BoundedCache:
    """LRU map of device tables (LUT stacks, index arrays) with at most `cap` entries.  Entries
    touched while a hipGraph is being captured are pinned and never evicted: a captured graph
    keeps reading their device memory on every replay, so freeing them would let the caching
    allocator hand that memory to someone else under the graph."""

    def __init__(self, cap: int, capturing):
        from collections import OrderedDict

        self.cap, self._capturing = cap, capturing
        self._d = OrderedDict()
        self._pinned = {}

    def get(self, key):
        if key in self._pinned:
            return self._pinned[key]
        v = self._d.get(key)
        if v is not None:
            self._d.move_to_end(key)
            if self._capturing():
                self._pinned[key] = self._d.pop(key)
        return v

    def put(self, key, value):
        if self._capturing():
            self._pinned[key] = value
            return
        self._d[key] = value
        self._d.move_to_end(key)
        while len(self._d) > self.cap:
            self._d.popitem(last=False)

    def __len__(self):
        return len(self._d) + len(self._pinned)


class _LayerPlan:
    """The device tables of one deep DAG (a division, an overflowing sub) on one operand shape: ONE stack of
    every LUT the DAG can ask for, the same for all its layers, and per distinct layer the int32 array of each
    row's index into that stack.  A layer is told apart by (K, the stack positions of its requests), so the second
    call on operands of the same shape finds every array and uploads nothing, however many layers the DAG has;
    _DeviceOps._tables, one stack per layer in an LRU, cannot promise that beyond its capacity."""

    def __init__(self, ops: "_DeviceOps", luts):
        self.luts = list(luts)
        self.position = {id(lut): i for i, lut in enumerate(self.luts)}
        self.stack = ops.from_host(np.stack([lut.acc for lut in self.luts]))
        self.indexes = {}

    def serves(self, luts) -> bool:
        return len(luts) == len(self.luts) and all(a is b for a, b in zip(luts, self.luts))

    def tables(self, ops: "_DeviceOps", K, lut_of_request, luts):
        where = tuple(self.position[id(luts[li])] for li in lut_of_request)
        idx = self.indexes.get((K, where))
        if idx is None:
            idx = ops.index_from_host(np.repeat(np.asarray(where, dtype=np.int32), K))
            self.indexes[(K, where)] = idx
        return self.stack, len(self.luts), idx


class _DeviceOps:
    """torch int64 tensors resident on the engine's GPU between layers; the LWE arithmetic runs in
    the engine's own kernels (lwe_ops.hip), torch only allocates, slices and copies."""

    CACHE_ENTRIES = 256  # distinct layer tables kept on the device (a FheUint32 multiply uses 11)
    PLAN_ENTRIES = 8     # table plans kept on the device: one per (deep DAG, blocks, K, operand shape)

    def __init__(self, sk: "ServerKey"):
        import torch

        self.torch = torch
        self.sk = sk
        self.eng = sk.shortint.engine
        self.device = torch.device("cuda", self.eng.device)
        capturing = torch.cuda.is_current_stream_capturing
        self._lut_dev = _BoundedCache(self.CACHE_ENTRIES, capturing)
        # LUT stacks and per-row LUT index arrays of the layers seen so far (bounded LRU)
        self._stacks = _BoundedCache(self.CACHE_ENTRIES, capturing)
        # the table plans of the deep DAGs (division, overflowing sub), one per operand shape (bounded LRU)
        self._plans = _BoundedCache(self.PLAN_ENTRIES, capturing)
        self._plan = None
        self._scratch = None

    def zeros(self, k, b, s):
        return self.torch.zeros((k, b, s), dtype=self.torch.int64, device=self.device)

    def roll(self, data, shift):
        return self.torch.roll(data, shift, dims=1) if shift else data

    def to_host(self, data):
        return data.cpu().numpy().view(np.uint64)

    def from_host(self, data):
        return self.torch.from_numpy(np.ascontiguousarray(data).view(np.int64)).to(self.device)

    def index_from_host(self, idx):
        """an int32 LUT-index array of a table plan: the other host-to-device copy a deep DAG makes"""
        return self.torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(self.device)

    def plan(self, key, luts):
        """Context of one deep DAG: while it is open every batched KS+PBS takes its tables from the _LayerPlan
        of `key` (made and uploaded the first time the key is seen) and not from _tables.  luts: every LUT the
        DAG can ask for, in a fixed order."""
        from contextlib import contextmanager

        @contextmanager
        def scope():
            plan = self._plans.get(key)
            if plan is None or not plan.serves(luts):
                plan = _LayerPlan(self, luts)
                self._plans.put(key, plan)
            outer, self._plan = self._plan, plan
            try:
                yield plan
            finally:
                self._plan = outer
        return scope()

    def copy_block(self, dst, j, src, i):
        dst.data[:, j, :].copy_(src.data[:, i, :])

    def set_trivial(self, rb, j, body):
        rb.data[:, j, :].zero_()
        rb.data[:, j, -1] = int(np.uint64(body).view(np.int64))

    def _row_ptr(self, rb, j, word=0):
        d = rb.data
        return d.data_ptr() + 8 * (j * d.shape[2] + word), d.shape[1] * d.shape[2]

    def mul_add(self, dst, j, scalar, src, i):
        yp, ys = self._row_ptr(dst, j)
        xp, xs = self._row_ptr(src, i) if src is not None else (None, 0)
        self.eng.lwe_scalar_mul_add_async(yp, xp, scalar, dst.count, dst.data.shape[2], ys, xs)

    def lut(self, lut):
        t = self._lut_dev.get(id(lut))
        if t is None or t[0] is not lut:
            t = (lut, self.from_host(lut.acc))
            self._lut_dev.put(id(lut), t)
        return t[1]

    def trivial_pbs(self, rb, j, lut):
        bp, stride = self._row_ptr(rb, j, rb.data.shape[2] - 1)
        self.eng.trivial_pbs_async(bp, rb.count, stride, self.lut(lut))

    def _layer_tables(self, todo, luts):
        """Device LUT stack and LUT-index array of a layer, uploaded the first time its shape is
        seen: the DAG repeats the same layers for every multiply, so a steady-state multiply does
        no host-to-device copy (nothing stalls the stream between launches, and the whole DAG can
        be captured into one hipGraph)."""
        return self._tables(todo[0][0].count, [li for _, _, li in todo], luts)

    def _tables(self, K, lut_of_request, luts):
        key =(K, tuple(id(lut) for lut in luts), tuple(lut_of_request) if len(luts) > 1 else ())
        hit = self._stacks.get(key)
        if hit is None or any(a is not b for a, b in zip(hit[0], luts)):
            d_luts = self.from_host(np.stack([lut.acc for lut in luts]))
            idx = None
            if len(luts) > 1:
                li = np.repeat(np.asarray(lut_of_request, dtype=np.int32), K)
                idx = self.torch.from_numpy(li).to(self.device)
            hit = (list(luts), d_luts, idx)
            self._stacks.put(key, hit)
        return hit[1], hit[2]

    def rows(self, n, s):
        return self.torch.empty((n, s), dtype=self.torch.int64, device=self.device)

    def block(self, rb, j):
        return rb.data[:, j, :]

    TERMS = 4  # TFHE_MI355_BLOCK_OP_TERMS

    def block_layer(self, ops):
        """_HostOps.block_layer on the device: one lwe_block_layer_async call (one launch up to 32 ops).  An op
        with more than 4 terms (the sums of eq / ne over up to msg * carry - 1 blocks) goes on in place in a
        further call per 3 terms, after the first: calls on one stream run in order, the ops of one call do not."""
        if not ops:
            return
        rows, words = ops[0][0].shape
        more = ops
        first = True
        while more:
            table, rest = [], []
            for dst, body_add, terms in more:
                assert dst.shape == (rows, words) and dst.stride(1) == 1
                head = terms[:self.TERMS] if first else [(dst, 1)] + terms[:self.TERMS - 1]
                tail = terms[self.TERMS:] if first else terms[self.TERMS - 1:]
                table.append((dst.data_ptr(), dst.stride(0), body_add if first else 0,
                              [(src.data_ptr(), src.stride(0), scalar) for src, scalar in head]))
                if tail:
                    rest.append((dst, 0, tail))
            self.eng.lwe_block_layer_async(table, rows, words)
            more, first = rest, False

    def clear_block_layer(self, ops):
        """_HostOps.clear_block_layer on the device: one lwe_clear_block_layer_async call (one launch up to 25
        ops).  The clear operands and the index array are read and written on the device, so the table holds
        addresses only.  Terms beyond 4 go on in place through block_layer, after the call."""
        if not ops:
            return
        rows, words = ops[0][0].shape
        table, rest = [], []
        for dst, body_add, terms, c in ops:
            assert dst.shape == (rows, words) and dst.stride(1) == 1
            clear = dict(negate=c["negate"], shift=c["shift"], bits=c["bits"], scale=c["scale"], lut_base=c["lut_base"])
            if c["rows"] is not None:
                clear["d_clear"] = c["rows"].on_device(self).data_ptr()
            if c["index"] is not None:
                clear["d_lut_index"] = c["index"].data_ptr()
            table.append((dst.data_ptr(), dst.stride(0), body_add,
                          [(src.data_ptr(), src.stride(0), scalar) for src, scalar in terms[:self.TERMS]], clear))
            if terms[self.TERMS:]:
                rest.append((dst, 0, [(dst, 1)] + terms[self.TERMS:]))
        self.eng.lwe_clear_block_layer_async(table, rows, words)
        if rest:
            self.block_layer(rest)

    def index_rows(self, n):
        return self.torch.empty(n, dtype=self.torch.int32, device=self.device)

    def _stack(self, luts):
        """the device stack of a layer's LUTs, uploaded the first time the list is seen"""
        key = ("stack",) + tuple(id(lut) for lut in luts)
        hit = self._stacks.get(key)
        if hit is None or any(a is not b for a, b in zip(hit[0], luts)):
            hit = (list(luts), self.from_host(np.stack([lut.acc for lut in luts])))
            self._stacks.put(key, hit)
        return hit[1]

    def pbs_buffer_indexed(self, x, luts, idx):
        """batched KS+PBS of the rows of x, row r with LUT idx[r] of `luts` (a device int32 array the block layer
        wrote; None: the one LUT) -> new rows"""
        torch = self.torch
        n = x.shape[0]
        out = torch.empty_like(x)
        need = self.eng.ks_pbs_scratch_bytes(n)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.eng.keyswitch_programmable_bootstrap_async(x, out, self._stack(luts), len(luts), n, self._scratch,
                                                        d_lut_indexes=idx)
        return out

    def pbs_buffer(self, x, K, lut_of_request, luts):
        """batched KS+PBS of the rows of x (request q: rows [qK, (q+1)K), LUT lut_of_request[q]) -> new rows"""
        torch = self.torch
        n = x.shape[0]
        if self._plan is not None:
            d_luts, nluts, idx = self._plan.tables(self, K, lut_of_request, luts)
        else:
            (d_luts, idx), nluts = self._tables(K, lut_of_request, luts), len(luts)
        out = torch.empty_like(x)
        need = self.eng.ks_pbs_scratch_bytes(n)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.eng.keyswitch_programmable_bootstrap_async(x, out, d_luts, nluts, n, self._scratch,
                                                        d_lut_indexes=idx)
        return out

    def pbs_rows(self, todo, luts):
        torch = self.torch
        K = todo[0][0].count
        x = torch.cat([rb.data[:, j, :] for rb, j, _ in todo], dim=0)
        out = self.pbs_buffer(x, K, [li for _, _, li in todo], luts)
        for q, (rb, j, _) in enumerate(todo):
            rb.data[:, j, :].copy_(out[q * K:(q + 1) * K])
        return x.shape[0]


def propagation_refusal(msg: int, carry: int):
    """Why the Hillis-Steele carry propagation and the chunked sum cannot serve a modulus pair (None: they
    can).  The reference takes this branch only with 4 bits per block
    (is_eligible_for_parallel_single_carry_propagation, add.rs:448-462) and propagates block by block
    otherwise; that sequential branch is not implemented here.  The other conditions are the ones the
    branch's own arithmetic needs, each stated where it is used below."""
    total = msg * carry
    if msg < 2 or (total - 1) // (msg - 1) < 3:
        # unchecked_sum_ciphertexts_vec: a chunk of `fill` terms becomes 2 terms (message, carry), so with
        # fill < 3 the term list never gets shorter
        return "fewer than 3 full messages fit in a block, so the chunked sum of terms would never shrink"
    if total < 16:
        return ("message_modulus * carry_modulus < 16: the reference propagates carries sequentially here "
                "(add.rs:448-462), and only the Hillis-Steele branch is implemented")
    if OUTPUT_CARRY_PROPAGATED + 1 > msg:
        # _bivariate(lut_prefix): the right operand is a carry state (0, 1 or 2) in the message bits
        return "a carry state (0, 1, 2) does not fit in the message bits of the prefix-sum bivariate PBS"
    if OUTPUT_CARRY_PROPAGATED * msg + OUTPUT_CARRY_PROPAGATED >= total:
        # _bivariate(lut_prefix): left carry state * message_modulus + right carry state
        return "two carry states packed for the prefix-sum bivariate PBS overflow the block"
    if (carry - 1) + (msg - 1) >= 2 * msg:
        # full_propagate / the sum's last step: extracted carries (degree carry_modulus - 1) are added to
        # extracted messages, and the single-carry propagation takes degrees below 2 * message_modulus
        return ("carry_modulus > message_modulus: an extracted carry added to a message can exceed one carry "
                "bit, which the single-carry propagation does not take")
    return None


def mul_refusal(msg: int, carry: int):
    """Why unchecked_mul cannot serve a pair the propagation can: the bivariate product PBS packs two full
    messages, lhs * message_modulus + rhs, into one block."""
    if (msg - 1) * msg + (msg - 1) >= msg * carry:
        return "carry_modulus < message_modulus: two messages packed for the bivariate product PBS overflow the block"
    return None


def bivariate_refusal(msg: int, carry: int):
    """Why a bivariate PBS layer (bitand / bitor / bitxor, eq / ne, zero_out_if of the cmux) cannot serve a pair:
    the operands are packed lhs * message_modulus + rhs into one block (bivariate_pbs.rs:167-182)."""
    if carry < msg:
        return "carry_modulus < message_modulus: two messages packed for a bivariate PBS overflow the block"
    return None


def comparison_refusal(msg: int, carry: int):
    """Comparator::new (comparator.rs:52-56)."""
    if msg * carry < 16:
        return "message_modulus * carry_modulus < 16: at least 4 bits of space (message + carry) are required to compare"
    return None


def barrel_shifter_refusal(msg: int, carry: int):
    """barrel_shifter's assert (radix_parallel/shift.rs:334-337): the mux input control | b | a takes 3 bits."""
    if (msg.bit_length() - 1) + (carry.bit_length() - 1) < 3:
        return "fewer than 3 bits (message + carry) in a block: the barrel shifter's mux input does not fit"
    return None


BORROW_NONE, BORROW_GENERATED, BORROW_PROPAGATED = 0, 1, 2   # radix_parallel/sub.rs:11-19


def overflowing_sub_refusal(msg: int, carry: int):
    """Why unsigned_overflowing_sub cannot serve a modulus pair (None: it can).  Only the Hillis-Steele branch of
    unsigned_overflowing_propagate_subtraction_borrow (sub.rs:397-421) is implemented; the conditions are the ones
    its arithmetic needs, each stated where it is used in _overflowing_sub_steps."""
    total = msg * carry
    if total < 16:
        return ("message_modulus * carry_modulus < 16: the reference propagates borrows sequentially here "
                "(add.rs:448-462), and only the Hillis-Steele branch is implemented")
    if 2 * msg - 1 >= total:
        # lhs - rhs + message_modulus: a block of the difference takes one carry bit
        return "carry_modulus < 2: a block of the difference, in 0 .. 2 * message_modulus - 1, overflows the block"
    if BORROW_PROPAGATED + 1 > msg:
        # the prefix sum's right operand is a borrow state (0, 1 or 2) in the message bits
        return "a borrow state (0, 1, 2) does not fit in the message bits of the prefix-sum bivariate PBS"
    if BORROW_PROPAGATED * msg + BORROW_PROPAGATED >= total:
        # the prefix sum packs left borrow state * message_modulus + right borrow state
        return "two borrow states packed for the prefix-sum bivariate PBS overflow the block"
    return None


def div_refusal(msg: int, carry: int):
    """Why the unsigned long division (div_mod.rs:92-492) cannot serve a modulus pair (None: it can): the
    conditions its own arithmetic needs, each stated where it is used in _unchecked_div_rem."""
    total = msg * carry
    if msg < 2 or msg & (msg - 1):
        # the loop goes bit by bit and trims the divisor at a bit boundary (div_mod.rs:125-129)
        return "the message modulus is not a power of two: the loop trims and shifts whole bits"
    sub = overflowing_sub_refusal(msg, carry)
    if sub:
        return sub                                    # the overflowing sub of every iteration
    if (msg - 1) * msg + (msg - 1) >= total:
        # R << 1: unchecked_scalar_left_shift packs previous * message_modulus + current (scalar_shift.rs:603-615)
        return "carry_modulus < message_modulus: two messages packed for the shift's bivariate PBS overflow the block"
    if 2 * (msg - 1) + msg >= total:
        # remainder1 + remainder2 - divisor + message_modulus: the degree the bookkeeping gives the difference
        return "the degree of remainder1 + remainder2 - divisor, 3 * message_modulus - 2, overflows the block"
    if 3 * (msg - 1) + 2 >= total:
        # the zero-outs pack block * 3 + overflow_sum, overflow_sum = overflowed + upper blocks non-zero <= 2
        return "a message packed with factor 3 over the overflow sum (0, 1, 2) overflows the block"
    if msg + 1 >= total:
        # merge_overflow_flags packs overflowed * message_modulus + upper blocks non-zero
        return "the two overflow flags packed for the quotient bit overflow the block"
    return None


IS_INFERIOR, IS_EQUAL, IS_SUPERIOR = 0, 1, 2   # comparator.rs:43-45
_NEG1 = (1 << 64) - 1


def _after_bitand(a: int, b: int) -> int:    # shortint/ciphertext/mod.rs:195-197
    return min(a, b)


def _after_bitor(a: int, b: int) -> int:     # :181-193
    hi, lo = max(a, b), min(a, b)
    return max(hi | i for i in range(lo + 1))


def _after_bitxor(a: int, b: int) -> int:    # :166-179
    hi, lo = max(a, b), min(a, b)
    return max([hi] + [hi ^ i for i in range(lo + 1)])


class ServerKey:
    """integer ServerKey (integer/server_key/mod.rs) over a shortint ServerKey with the GPU engine."""

    def __init__(self, shortint_key: ShortintServerKey):
        self.shortint = shortint_key
        p = shortint_key.parameters
        if shortint_key.pbs_order != KEYSWITCH_BOOTSTRAP:
            raise NotImplementedError("integer layer implemented for PBSOrder::KeyswitchBootstrap keys")
        self.p = p
        self.msg = p.message_modulus
        self.carry = p.carry_modulus
        self.lwe_size = p.big_lwe_dimension + 1
        self.pbs_count = 0
        self.launches = 0
        self.ops = _DeviceOps(self) if _is_gpu_engine(shortint_key.engine) else _HostOps(self)
        m = self.msg
        self.lut_message = self.shortint.generate_lookup_table(lambda x: x % m)
        self.lut_carry = self.shortint.generate_lookup_table(lambda x: x // m)
        self.lut_mul_lsb = self.generate_lookup_table_bivariate(lambda x, y: (x * y) % m)
        self.lut_mul_msb = self.generate_lookup_table_bivariate(lambda x, y: (x * y) // m)
        self.lut_gen_carry = self.shortint.generate_lookup_table(
            lambda x: OUTPUT_CARRY_GENERATED if x >= m else OUTPUT_CARRY_NONE)
        self.lut_gen_or_prop = self.shortint.generate_lookup_table(
            lambda x: OUTPUT_CARRY_GENERATED if x >= m else (OUTPUT_CARRY_PROPAGATED if x == m - 1
                                                             else OUTPUT_CARRY_NONE))
        self.lut_prefix = self.generate_lookup_table_bivariate(
            lambda msb, lsb: lsb if msb == OUTPUT_CARRY_PROPAGATED else msb)
        self.propagation_refusal = propagation_refusal(m, self.carry)
        self.mul_refusal = self.propagation_refusal or mul_refusal(m, self.carry)
        self.bivariate_refusal = bivariate_refusal(m, self.carry)
        self.comparison_refusal = comparison_refusal(m, self.carry)
        self.barrel_shifter_refusal = barrel_shifter_refusal(m, self.carry)
        self.overflowing_sub_refusal = overflowing_sub_refusal(m, self.carry)
        self.div_refusal = div_refusal(m, self.carry)
        self.bits = m.bit_length() - 1          # message bits per block
        self._luts = {}   # the LUTs of neg .. min / max, built on first use: (name, ...) -> LookupTable

    def _require(self, op: str, refusal):
        """The carry-propagating entry points refuse a parameter set they cannot serve before the
        first PBS or kernel launch (the key itself is built for every set: the WoP-PBS layer uses one)."""
        if refusal:
            raise NotImplementedError(f"integer {op}: {self.p.name or 'parameters'} (message modulus {self.msg}, "
                                      f"carry modulus {self.carry}) is not supported: {refusal}")

    # -- lookup tables -----------------------------------------------------------------------
    def generate_lookup_table_bivariate(self, f) -> LookupTable:
        """generate_lookup_table_bivariate (bivariate_pbs.rs:69-100), left scaling = message modulus."""
        m = self.msg
        return self.shortint.generate_lookup_table(lambda x: f((x // m) % m, (x % m) % m))

    def generate_lookup_table_bivariate_with_factor(self, f, factor: int) -> LookupTable:
        """bivariate_pbs.rs:71-96: the left operand is scaled by `factor`, not by the message modulus."""
        m = self.msg
        return self.shortint.generate_lookup_table(lambda x: f((x // factor) % m, (x % factor) % m))

    # -- block primitives (shortint) -----------------------------------------------------------
    def _trivial_pbs(self, rb: RadixBatch, j: int, lut: LookupTable):
        """trivial_pbs_assign (shortint/server_key/mod.rs:763-781) for every ciphertext of the batch."""
        self.ops.trivial_pbs(rb, j, lut)

    def _set_trivial(self, rb: RadixBatch, j: int, value: int = 0):
        """create_trivial_assign (shortint server_key create_trivial)."""
        self.ops.set_trivial(rb, j, (value % (self.msg * self.carry)) * self.p.delta)
        rb.degree[j] = value
        rb.noise[j] = NOISE_ZERO

    def _add_block(self, dst: RadixBatch, j: int, src: RadixBatch, i: int):
        """shortint unchecked_add_assign: LWE add, degree and noise level add."""
        self.ops.mul_add(dst, j, 1, src, i)
        dst.degree[j] += src.degree[i]
        dst.noise[j] += src.noise[i]

    def _scalar_mul_block(self, rb: RadixBatch, j: int, s: int):
        self.ops.mul_add(rb, j, s, None, 0)
        rb.degree[j] *= s
        rb.noise[j] *= s

    def _bivariate(self, layer: _PbsLayer, left: RadixBatch, j: int, right: RadixBatch, i: int, lut: LookupTable):
        """unchecked_apply_lookup_table_bivariate_assign (bivariate_pbs.rs:167-182):
        left = left * message_modulus + right, then the LUT (queued on `layer`)."""
        assert right.degree[i] + 1 <= self.msg
        self._scalar_mul_block(left, j, self.msg)
        self._add_block(left, j, right, i)
        layer.add(left, j, lut)

    # -- radix helpers -------------------------------------------------------------------------
    def create_trivial_zero(self, count: int, num_blocks: int) -> RadixBatch:
        return RadixBatch(self.ops.zeros(count, num_blocks, self.lwe_size), [0] * num_blocks,
                          [NOISE_ZERO] * num_blocks)

    def blockshift(self, ct: RadixBatch, shift: int) -> RadixBatch:
        """radix/scalar_mul.rs:345-355: rotate_right(shift), low blocks trivial zeros."""
        res = ct.clone()
        nb = ct.num_blocks
        s = shift % nb if nb else 0
        res.data = self.ops.roll(res.data, s)
        res.degree = res.degree[nb - s:] + res.degree[:nb - s]
        res.noise = res.noise[nb - s:] + res.noise[:nb - s]
        for j in range(min(shift, nb)):
            self._set_trivial(res, j, 0)
        return res

    def unchecked_add_assign(self, lhs: RadixBatch, rhs: RadixBatch):
        for j in range(lhs.num_blocks):
            self._add_block(lhs, j, rhs, j)

    # -- carry propagation (Hillis-Steele branch) ------------------------------------------
    def _propagate_single_carry_low_latency(self, ct: RadixBatch):
        """propagate_single_carry_parallelized_low_latency (add.rs:518-537)."""
        nb = ct.num_blocks
        layer = _PbsLayer(self)
        gp = ct.clone()
        for j in range(nb):   # generate_init_carry_array (add.rs:724-771)
            layer.add(gp, j, self.lut_gen_carry if j == 0 else self.lut_gen_or_prop)
        layer.flush()
        # compute_prefix_sum_hillis_steele (add.rs:572-603)
        num_steps = (nb - 1).bit_length() if nb > 1 else 0
        space = 1
        for _ in range(num_steps):
            step = gp.clone()
            for b in range(space, nb):
                self._bivariate(layer, step, b, gp, b - space, self.lut_prefix)
            layer.flush()
            for b in range(space, nb):
                self.ops.copy_block(gp, b, step, b)
                gp.degree[b] = step.degree[b]
                gp.noise[b] = step.noise[b]
            space *= 2
        # compute_carry_propagation_parallelized_low_latency (add.rs:544-570): the last carry is
        # swapped out for a trivial zero, then rotate_right(1)
        carries = gp
        self._set_trivial(carries, nb - 1, 0)
        carries.data = self.ops.roll(carries.data, 1)
        carries.degree = carries.degree[-1:] + carries.degree[:-1]
        carries.noise = carries.noise[-1:] + carries.noise[:-1]
        for j in range(nb):
            self._add_block(ct, j, carries, j)
            layer.add(ct, j, self.lut_message)
        layer.flush()

    def _unchecked_add_assign_low_latency(self, lhs: RadixBatch, rhs: RadixBatch):
        """unchecked_add_assign_parallelized_low_latency (add.rs:487-507)."""
        assert all(a + b < self.msg * 2 for a, b in zip(lhs.degree, rhs.degree))
        self.unchecked_add_assign(lhs, rhs)
        self._propagate_single_carry_low_latency(lhs)

    def full_propagate(self, ct: RadixBatch):
        """full_propagate_parallelized = partial_propagate_parallelized(ct, 0) (mod.rs:88-155)."""
        self._require("full_propagate", self.propagation_refusal)
        nb = ct.num_blocks
        carries = ct.clone()
        layer = _PbsLayer(self)
        for j in range(nb):
            layer.add(ct, j, self.lut_message)
        for j in range(nb - 1):
            layer.add(carries, j, self.lut_carry)
        layer.flush()
        self._set_trivial(carries, nb - 1, 0)
        carries.data = self.ops.roll(carries.data, 1)
        carries.degree = carries.degree[-1:] + carries.degree[:-1]
        carries.noise = carries.noise[-1:] + carries.noise[:-1]
        self._unchecked_add_assign_low_latency(ct, carries)

    def add_assign_parallelized(self, lhs: RadixBatch, rhs: RadixBatch):
        """add.rs:206-242 (Hillis-Steele branch)."""
        self._require("add_assign_parallelized", self.propagation_refusal)
        if not rhs.block_carries_are_empty(self.msg):
            rhs = rhs.clone()
            self.full_propagate(rhs)
        if not lhs.block_carries_are_empty(self.msg):
            self.full_propagate(lhs)
        self._unchecked_add_assign_low_latency(lhs, rhs)

    # -- sum of terms ------------------------------------------------------------------------
    def unchecked_sum_ciphertexts_vec(self, cts: list) -> RadixBatch | None:
        """unchecked_sum_ciphertexts_vec_parallelized (add.rs:783-960)."""
        self._require("unchecked_sum_ciphertexts_vec", self.propagation_refusal)
        if not cts:
            return None
        if len(cts) == 1:
            return cts[0]
        nb = cts[0].num_blocks
        if len(cts) == 2:
            res = cts[0].clone()
            self.add_assign_parallelized(res, cts[1])
            return res
        assert all(c.block_carries_are_empty(self.msg) for c in cts)
        total = self.msg * self.carry
        fill = (total - 1) // (self.msg - 1)
        cts = list(cts)
        while len(cts) > fill:
            nchunks = len(cts) // fill
            rem = cts[nchunks * fill:]
            layer = _PbsLayer(self)
            outs = []
            for c in range(nchunks):
                chunk = cts[c * fill:(c + 1) * fill]
                s = chunk[0].clone()
                first_where, last_where = nb - 1, 0
                for a in chunk[1:]:
                    nz = [j for j in range(nb) if a.degree[j] != 0]
                    first_add = nz[0] if nz else nb
                    last_add = nz[-1] if nz else nb - 1
                    first_where = min(first_where, first_add)
                    last_where = max(last_where, last_add)
                    for j in range(first_add, last_add + 1):
                        self._add_block(s, j, a, j)
                carry = s.clone()
                for j in range(first_where, last_where + 1):
                    layer.add(s, j, self.lut_message)
                start = first_where
                end = last_where - 1 if last_where == nb - 1 else last_where
                for j in range(start, end + 1):
                    layer.add(carry, j, self.lut_carry)
                outs.append((s, carry, start, end))
            layer.flush()
            new = []
            for s, carry, start, end in outs:
                for j in range(0, start):
                    self._set_trivial(carry, j, 0)
                for j in range(end + 1, nb):
                    self._set_trivial(carry, j, 0)
                carry.data = self.ops.roll(carry.data, 1)
                carry.degree = carry.degree[-1:] + carry.degree[:-1]
                carry.noise = carry.noise[-1:] + carry.noise[:-1]
                new += [s, carry]
            cts = new + rem
        result = cts[0].clone()
        for t in cts[1:]:
            self.unchecked_add_assign(result, t)
        carry = result.clone()
        layer = _PbsLayer(self)
        for j in range(nb):
            layer.add(result, j, self.lut_message)
        for j in range(nb - 1):
            layer.add(carry, j, self.lut_carry)
        layer.flush()
        self._set_trivial(carry, nb - 1, 0)
        carry.data = self.ops.roll(carry.data, 1)
        carry.degree = carry.degree[-1:] + carry.degree[:-1]
        carry.noise = carry.noise[-1:] + carry.noise[:-1]
        self.add_assign_parallelized(result, carry)
        assert result.block_carries_are_empty(self.msg)
        return result

    def to_device(self, rb: RadixBatch) -> RadixBatch:
        """Host RadixBatch (from ClientKey.encrypt) -> this key's residency."""
        return RadixBatch(self.ops.from_host(rb.data), list(rb.degree), list(rb.noise))

    def to_host(self, rb: RadixBatch) -> RadixBatch:
        return RadixBatch(self.ops.to_host(rb.data) if not isinstance(rb.data, np.ndarray) else rb.data,
                          list(rb.degree), list(rb.noise))

    # -- multiplication ------------------------------------------------------------------------
    def unchecked_mul(self, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        """unchecked_mul_assign_parallelized (mul.rs:300-414)."""
        self._require("unchecked_mul", self.mul_refusal)
        lhs, rhs = self._resident(lhs), self._resident(rhs)
        if rhs.holds_boolean_value() or lhs.holds_boolean_value():
            raise NotImplementedError("boolean-valued operand (zero_out_if_condition_is_false path)")
        nb = lhs.num_blocks
        layer = _PbsLayer(self)
        terms = []
        rhs_nz = [i for i in range(nb) if rhs.degree[i] != 0]
        for i in rhs_nz:                       # message part: (x * y) % modulus
            res = self.blockshift(lhs, i)
            for j in range(i, nb):
                if res.degree[j] != 0:
                    self._bivariate(layer, res, j, rhs, i, self.lut_mul_lsb)
            terms.append(res)
        if self.msg > 2:                       # carry part: (x * y) / modulus, shifted one more
            for i in rhs_nz:
                res = self.blockshift(lhs, i + 1)
                for j in range(i + 1, nb):
                    if res.degree[j] != 0:
                        self._bivariate(layer, res, j, rhs, i, self.lut_mul_msb)
                terms.append(res)
        layer.flush()                          # every bivariate PBS of the product in one launch
        out = self.unchecked_sum_ciphertexts_vec(terms)
        return out if out is not None else self.create_trivial_zero(lhs.count, nb)

    def _resident(self, rb: RadixBatch) -> RadixBatch:
        if isinstance(rb.data, np.ndarray) and isinstance(self.ops, _DeviceOps):
            return self.to_device(rb)
        return rb

    def mul_parallelized(self, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        """mul.rs:553-590."""
        self._require("mul_parallelized", self.mul_refusal)
        lhs, rhs = self._resident(lhs), self._resident(rhs)
        lhs = lhs.clone()
        if not rhs.block_carries_are_empty(self.msg):
            rhs = rhs.clone()
            self.full_propagate(rhs)
        if not lhs.block_carries_are_empty(self.msg):
            self.full_propagate(lhs)
        return self.unchecked_mul(lhs, rhs)

    # ---- neg, sub, bitwise ops, comparisons, cmux, min / max ----------------------------------------------
    # Mirrors of the reference functions named in each docstring, for K unsigned operands at once.  Every PBS
    # layer is a fused _PbsLayer (flush_fused): the block arithmetic the reference does between two layers --
    # pack_block_chunk, the LWE subtraction of compare_block_assign, 4 * high + low of the sign tree, the sums
    # of eq / ne, the bivariate packing -- is the prepare op of the request that consumes it.  A BooleanBlock
    # is a one-block RadixBatch of degree <= 1.  Out of scope: signed integers, signed div / abs and the smart_*
    # forms.
    def _lut(self, key, f, bivariate: bool = False, factor: int = 0) -> LookupTable:
        """One LookupTable object per function for the life of the key: the device caches go by identity.  factor:
        a bivariate LUT whose left operand is scaled by it."""
        t = self._luts.get(key)
        if t is None:
            if factor:
                t = self.generate_lookup_table_bivariate_with_factor(f, factor)
            else:
                t = self.generate_lookup_table_bivariate(f) if bivariate else self.shortint.generate_lookup_table(f)
            self._luts[key] = t
        return t

    def _new(self, count: int, num_blocks: int) -> RadixBatch:
        """a batch whose blocks are all written before they are read"""
        return RadixBatch(self.ops.rows(count * num_blocks, self.lwe_size).reshape(count, num_blocks, self.lwe_size),
                          [0] * num_blocks, [NOISE_ZERO] * num_blocks)

    def _clean(self, ct: RadixBatch) -> RadixBatch:
        """the operand itself with empty carries, or a propagated clone (the default forms' preamble)"""
        ct = self._resident(ct)
        if ct.block_carries_are_empty(self.msg):
            return ct
        ct = ct.clone()
        self.full_propagate(ct)
        return ct

    def unchecked_neg(self, ct: RadixBatch) -> RadixBatch:
        """unchecked_neg / unchecked_neg_assign (radix/neg.rs:39-73) over shortint
        unchecked_neg_assign_with_correcting_term (shortint/server_key/neg.rs:223-246): block j becomes
        (z - z_b) * delta - block, z = max(ceil((degree + z_b) / msg), 1) * msg, z_b the carry of the correcting
        term of the block before.  One block op per block, no PBS."""
        ct = self._resident(ct)
        res = self._new(ct.count, ct.num_blocks)
        ops, z_b = [], 0
        for j in range(ct.num_blocks):
            degree = ct.degree[j] + z_b                        # unchecked_scalar_add_assign(block, z_b)
            z = max(-(-degree // self.msg), 1) * self.msg
            ops.append((self.ops.block(res, j), (z - z_b) * self.p.delta, [(self.ops.block(ct, j), _NEG1)]))
            res.degree[j] = z - z_b
            res.noise[j] = ct.noise[j]
            z_b = z // self.msg
        self.ops.block_layer(ops)
        return res

    def neg_parallelized(self, ct: RadixBatch) -> RadixBatch:
        """radix_parallel/neg.rs:77-100 (the branch of is_eligible_for_parallel_single_carry_propagation)."""
        self._require("neg_parallelized", self.propagation_refusal)
        res = self.unchecked_neg(self._clean(ct))
        self._propagate_single_carry_low_latency(res)
        return res

    def unchecked_sub_assign(self, lhs: RadixBatch, rhs: RadixBatch):
        """radix/sub.rs:80-86."""
        self.unchecked_add_assign(lhs, self.unchecked_neg(rhs))

    def sub_assign_parallelized(self, lhs: RadixBatch, rhs: RadixBatch):
        """radix_parallel/sub.rs:206-243, the eligible branch: unchecked_neg, then
        unchecked_add_assign_parallelized_low_latency.  lhs must be resident (it is assigned)."""
        self._require("sub_assign_parallelized", self.propagation_refusal)
        rhs = self._clean(rhs)
        if not lhs.block_carries_are_empty(self.msg):
            self.full_propagate(lhs)
        self._unchecked_add_assign_low_latency(lhs, self.unchecked_neg(rhs))

    def sub_parallelized(self, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        """radix_parallel/sub.rs:162-169."""
        self._require("sub_parallelized", self.propagation_refusal)
        res = self._resident(lhs).clone()
        self.sub_assign_parallelized(res, rhs)
        return res

    # -- bitwise --------------------------------------------------------------------------------------------
    _BITOPS = {"bitand": (lambda x, y: x & y, _after_bitand), "bitor": (lambda x, y: x | y, _after_bitor),
               "bitxor": (lambda x, y: x ^ y, _after_bitxor)}

    def _unchecked_bitop_assign(self, name: str, lhs: RadixBatch, rhs: RadixBatch):
        """unchecked_bit{and,or,xor}_assign_parallelized (radix_parallel/bitwise_op.rs:15-26, 180-191, 347-358)
        over shortint unchecked_evaluate_bivariate_function_assign (bivariate_pbs.rs:277-290): per block
        lhs * (rhs.degree + 1) + rhs, the LUT of that factor, then Degree::after_bit*.  One PBS layer."""
        self._require(f"unchecked_{name}_assign_parallelized", self.bivariate_refusal)
        f, after = self._BITOPS[name]
        rhs = self._resident(rhs)
        total, m = self.msg * self.carry, self.msg
        layer = _PbsLayer(self)
        degrees = []
        for j in range(lhs.num_blocks):
            factor = rhs.degree[j] + 1
            if lhs.degree[j] * factor + rhs.degree[j] >= total:
                raise ValueError(f"unchecked_{name}: block {j} (degrees {lhs.degree[j]}, {rhs.degree[j]}) cannot be "
                                 "packed for a bivariate PBS")
            lut = self._lut((name, factor), lambda x, f=f, k=factor: f((x // k) % m, (x % k) % m))
            degrees.append(after(lhs.degree[j], rhs.degree[j]))
            layer.add(lhs, j, lut, prepare=(0, [(lhs, j, factor), (rhs, j, 1)]))
        layer.flush()
        lhs.degree = degrees

    def _bitop(self, name: str, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        """bit{and,or,xor}_parallelized (bitwise_op.rs:129-169, 296-336, 463-503)."""
        self._require(f"{name}_parallelized", self.bivariate_refusal)
        lhs, rhs = self._clean(lhs), self._clean(rhs)
        res = lhs.clone()
        self._unchecked_bitop_assign(name, res, rhs)
        return res

    def unchecked_bitand_assign_parallelized(self, lhs, rhs):
        self._unchecked_bitop_assign("bitand", lhs, rhs)

    def unchecked_bitor_assign_parallelized(self, lhs, rhs):
        self._unchecked_bitop_assign("bitor", lhs, rhs)

    def unchecked_bitxor_assign_parallelized(self, lhs, rhs):
        self._unchecked_bitop_assign("bitxor", lhs, rhs)

    def bitand_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._bitop("bitand", lhs, rhs)

    def bitor_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._bitop("bitor", lhs, rhs)

    def bitxor_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._bitop("bitxor", lhs, rhs)

    def bitnot_parallelized(self, ct: RadixBatch) -> RadixBatch:
        """bitwise_op.rs:540-562: (!x) % message_modulus on every block."""
        res = self._resident(ct).clone()
        if not res.block_carries_are_empty(self.msg):
            self.full_propagate(res)
        m = self.msg
        lut = self._lut(("bitnot",), lambda x: (~x) % m)
        layer = _PbsLayer(self)
        for j in range(res.num_blocks):
            layer.add(res, j, lut)
        layer.flush()
        return res

    # -- eq / ne ----------------------------------------------------------------------------------------------
    def _reduce_block_comparisons(self, blocks: list, all_true: bool) -> RadixBatch:
        """are_all_comparisons_block_true (scalar_comparison.rs:147-191) and the reduction of
        unchecked_ne_parallelized (comparison.rs:55-83): blocks of 0 / 1 are summed in chunks of
        msg * carry - 1, a LUT tells whether the sum is the chunk's length (eq) or non-zero (ne); one PBS layer
        per pass.  blocks: [(batch, block)]; returns the one-block batch."""
        layer = _PbsLayer(self)
        (rb, _), = self._join(layer, self._reduce_block_comparisons_steps(layer, blocks, all_true))
        assert rb.num_blocks == 1   # one block in, or the single chunk of the last pass
        return rb

    def _reduce_block_comparisons_steps(self, layer: _PbsLayer, blocks: list, all_true: bool):
        """The loop of _reduce_block_comparisons as a branch of _join: it queues a pass on `layer` and yields where
        the reference waits for it.  Returns the (batch, block) left; a single block comes back as it is."""
        count = blocks[0][0].count
        max_value = self.msg * self.carry - 1
        while len(blocks) > 1:
            chunks = [blocks[c:c + max_value] for c in range(0, len(blocks), max_value)]
            out = self._new(count, len(chunks))
            for c, chunk in enumerate(chunks):
                n = len(chunk)
                lut = self._lut(("sum_is", n), lambda x, n=n: int(x == n)) if all_true else \
                    self._lut(("sum_non_zero",), lambda x: int(x != 0))
                layer.add(out, c, lut, prepare=(0, [(rb, j, 1) for rb, j in chunk]))
            yield
            blocks = [(out, c) for c in range(len(chunks))]
        return blocks[0]

    def _join(self, layer: _PbsLayer, *branches) -> list:
        """rayon::join / par_iter over branches that take several PBS passes each: pass k of every branch goes
        into the same batched launch.  A branch is a generator that queues its requests on `layer` and yields
        where it needs them done; what it returns is its result."""
        results, live = [None] * len(branches), dict(enumerate(branches))
        while live:
            for i, branch in list(live.items()):
                try:
                    next(branch)
                except StopIteration as done:
                    results[i] = done.value
                    del live[i]
            if layer.reqs:
                layer.flush()
        return results

    def _unchecked_equality(self, name: str, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        self._require(f"unchecked_{name}_parallelized", self.bivariate_refusal)
        lhs, rhs = self._resident(lhs), self._resident(rhs)
        assert lhs.num_blocks == rhs.num_blocks and lhs.num_blocks > 0
        eq = name == "eq"
        lut = self._lut((name,), (lambda x, y: int(x == y)) if eq else (lambda x, y: int(x != y)), bivariate=True)
        cmp = self._new(lhs.count, lhs.num_blocks)
        layer = _PbsLayer(self)
        for j in range(lhs.num_blocks):
            assert rhs.degree[j] < self.msg and lhs.degree[j] < self.msg
            layer.add(cmp, j, lut, prepare=(0, [(lhs, j, self.msg), (rhs, j, 1)]))
        layer.flush()
        return self._reduce_block_comparisons([(cmp, j) for j in range(cmp.num_blocks)], eq)

    def unchecked_eq_parallelized(self, lhs, rhs) -> RadixBatch:
        """radix_parallel/comparison.rs:10-33."""
        return self._unchecked_equality("eq", lhs, rhs)

    def unchecked_ne_parallelized(self, lhs, rhs) -> RadixBatch:
        """radix_parallel/comparison.rs:35-83."""
        return self._unchecked_equality("ne", lhs, rhs)

    def eq_parallelized(self, lhs, rhs) -> RadixBatch:
        """radix_parallel/comparison.rs:207-237."""
        self._require("eq_parallelized", self.bivariate_refusal)
        return self._unchecked_equality("eq", self._clean(lhs), self._clean(rhs))

    def ne_parallelized(self, lhs, rhs) -> RadixBatch:
        """radix_parallel/comparison.rs:239-269."""
        self._require("ne_parallelized", self.bivariate_refusal)
        return self._unchecked_equality("ne", self._clean(lhs), self._clean(rhs))

    # -- order ------------------------------------------------------------------------------------------------
    def _unchecked_compare(self, lhs: RadixBatch, rhs: RadixBatch):
        """Comparator::unchecked_compare_parallelized (comparator.rs:389-463): the sign block (batch, block) of
        lhs against rhs, IS_INFERIOR / IS_EQUAL / IS_SUPERIOR.  compare_block_assign (:193-220) is the true LWE
        subtraction, sign_lut, + 1 on the body; with carry >= msg it runs on pairs of blocks packed by
        pack_block_chunk (:182-187), so its PBS input is the one op  m * lhs_hi + lhs_lo - m * rhs_hi - rhs_lo.
        reduce_signs_parallelized (:257-280) is the tree of 4 * high + low -> comparison_reduction_lut."""
        assert lhs.num_blocks == rhs.num_blocks and lhs.num_blocks > 0
        nb, m = lhs.num_blocks, self.msg
        assert all(d < m for d in lhs.degree + rhs.degree)
        sign_lut = self._lut(("sign",), lambda x: int(x != 0))
        chunks = [[j] for j in range(nb)] if self.carry < m else [list(range(j, min(j + 2, nb))) for j in range(0, nb, 2)]
        signs = self._new(lhs.count, len(chunks))
        layer = _PbsLayer(self)
        for c, chunk in enumerate(chunks):
            if len(chunk) == 2:
                lo, hi = chunk
                terms = [(lhs, hi, m), (lhs, lo, 1), (rhs, hi, -m), (rhs, lo, -1)]
            else:
                terms = [(lhs, chunk[0], 1), (rhs, chunk[0], -1)]
            layer.add(signs, c, sign_lut, prepare=(0, terms), post_add=1)
        layer.flush()
        table = [IS_INFERIOR] * 5 + [IS_EQUAL] + [IS_SUPERIOR] * 5      # comparator.rs:81-100, index 4 * high + low
        reduction = self._lut(("sign_reduction",), lambda x: table[x] if x < len(table) else 0)
        blocks = [(signs, c) for c in range(len(chunks))]
        while len(blocks) != 1:
            out = self._new(lhs.count, len(blocks) // 2)
            for c in range(len(blocks) // 2):
                (low, lj), (high, hj) = blocks[2 * c], blocks[2 * c + 1]
                assert 4 * high.degree[hj] + low.degree[lj] < self.msg * self.carry
                layer.add(out, c, reduction, prepare=(0, [(high, hj, 4), (low, lj, 1)]))
            layer.flush()
            blocks = [(out, c) for c in range(len(blocks) // 2)] + (blocks[-1:] if len(blocks) % 2 else [])
        return blocks[0]

    _ORDER = {"gt": lambda x: x == IS_SUPERIOR, "ge": lambda x: x in (IS_EQUAL, IS_SUPERIOR),
              "lt": lambda x: x == IS_INFERIOR, "le": lambda x: x in (IS_EQUAL, IS_INFERIOR)}

    def _unchecked_order(self, name: str, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        """unchecked_{gt,ge,lt,le}_parallelized (comparator.rs:1079-1125): the sign, then map_sign_result
        (:957-971)."""
        self._require(f"unchecked_{name}_parallelized", self.comparison_refusal)
        lhs, rhs = self._resident(lhs), self._resident(rhs)
        sign, sj = self._unchecked_compare(lhs, rhs)
        res = self._new(lhs.count, 1)
        layer = _PbsLayer(self)
        layer.add(res, 0, self._lut(("sign_is", name), lambda x, f=self._ORDER[name]: int(f(x))),
                  prepare=(0, [(sign, sj, 1)]))
        layer.flush()
        return res

    def _order(self, name: str, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        """{gt,ge,lt,le}_parallelized (comparator.rs:1267-1393)."""
        self._require(f"{name}_parallelized", self.comparison_refusal)
        return self._unchecked_order(name, self._clean(lhs), self._clean(rhs))

    def unchecked_gt_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._unchecked_order("gt", lhs, rhs)

    def unchecked_ge_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._unchecked_order("ge", lhs, rhs)

    def unchecked_lt_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._unchecked_order("lt", lhs, rhs)

    def unchecked_le_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._unchecked_order("le", lhs, rhs)

    def gt_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._order("gt", lhs, rhs)

    def ge_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._order("ge", lhs, rhs)

    def lt_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._order("lt", lhs, rhs)

    def le_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._order("le", lhs, rhs)

    # -- select -----------------------------------------------------------------------------------------------
    def _zero_out_if(self, layer: _PbsLayer, ct: RadixBatch, cond: RadixBatch, cj: int, key, predicate) -> RadixBatch:
        """zero_out_if (radix_parallel/cmux.rs:281-316) on a clone of ct, its PBS requests queued on `layer`: a
        condition of degree 0 decides on the spot, blocks of degree 0 are skipped."""
        assert cond.degree[cj] < self.msg
        res = ct.clone()
        if cond.degree[cj] == 0:
            if predicate(0):
                for j in range(res.num_blocks):   # create_trivial_zero_assign_radix
                    self._set_trivial(res, j, 0)
            return res
        lut = self._lut(("zero_out_if", key), lambda block, c: 0 if predicate(c) else block, bivariate=True)
        for j in range(res.num_blocks):
            if res.degree[j] != 0:
                assert res.degree[j] < self.msg
                layer.add(res, j, lut, prepare=(0, [(res, j, self.msg), (cond, cj, 1)]))
        return res

    def _programmable_if_then_else(self, cond: RadixBatch, cj: int, true_ct: RadixBatch, false_ct: RadixBatch, key,
                                   predicate) -> RadixBatch:
        """unchecked_programmable_if_then_else_parallelized (cmux.rs:194-248), do_clean_message = true: both
        zero_out_if in one PBS layer (the reference joins them), then add and message_extract in a second."""
        layer = _PbsLayer(self)
        t = self._zero_out_if(layer, true_ct, cond, cj, (key, False), lambda x: not predicate(x))
        f = self._zero_out_if(layer, false_ct, cond, cj, (key, True), predicate)
        layer.flush()
        for j in range(t.num_blocks):
            layer.add(t, j, self.lut_message, prepare=(0, [(t, j, 1), (f, j, 1)]))
        layer.flush()
        return t

    def unchecked_if_then_else_parallelized(self, condition: RadixBatch, true_ct: RadixBatch,
                                            false_ct: RadixBatch) -> RadixBatch:
        """cmux.rs:7-25: condition is a BooleanBlock, a one-block batch of degree <= 1."""
        self._require("unchecked_if_then_else_parallelized", self.bivariate_refusal)
        condition, true_ct, false_ct = self._resident(condition), self._resident(true_ct), self._resident(false_ct)
        assert condition.num_blocks == 1 and condition.degree[0] <= 1 and true_ct.num_blocks == false_ct.num_blocks
        return self._programmable_if_then_else(condition, 0, true_ct, false_ct, "true", lambda x: x == 1)

    def if_then_else_parallelized(self, condition: RadixBatch, true_ct: RadixBatch, false_ct: RadixBatch) -> RadixBatch:
        """cmux.rs:72-97."""
        self._require("if_then_else_parallelized", self.bivariate_refusal)
        return self.unchecked_if_then_else_parallelized(condition, self._clean(true_ct), self._clean(false_ct))

    cmux_parallelized = if_then_else_parallelized   # cmux.rs:102-107

    # -- min / max ----------------------------------------------------------------------------------------------
    def _unchecked_min_or_max(self, name: str, lhs: RadixBatch, rhs: RadixBatch) -> RadixBatch:
        """Comparator::unchecked_min_or_max_parallelized (comparator.rs:849-875): the sign, then the programmable
        cmux on it (max keeps lhs where the sign is IS_SUPERIOR, min where it is IS_INFERIOR)."""
        self._require(f"unchecked_{name}_parallelized", self.comparison_refusal or self.bivariate_refusal)
        lhs, rhs = self._resident(lhs), self._resident(rhs)
        sign, sj = self._unchecked_compare(lhs, rhs)
        keep = IS_SUPERIOR if name == "max" else IS_INFERIOR
        return self._programmable_if_then_else(sign, sj, lhs, rhs, name, lambda x: x == keep)

    def unchecked_max_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._unchecked_min_or_max("max", lhs, rhs)

    def unchecked_min_parallelized(self, lhs, rhs) -> RadixBatch:
        return self._unchecked_min_or_max("min", lhs, rhs)

    def max_parallelized(self, lhs, rhs) -> RadixBatch:
        """comparator.rs:1395-1426."""
        self._require("max_parallelized", self.comparison_refusal or self.bivariate_refusal)
        return self._unchecked_min_or_max("max", self._clean(lhs), self._clean(rhs))

    def min_parallelized(self, lhs, rhs) -> RadixBatch:
        """comparator.rs:1428-1459."""
        self._require("min_parallelized", self.comparison_refusal or self.bivariate_refusal)
        return self._unchecked_min_or_max("min", self._clean(lhs), self._clean(rhs))

    # ---- clear operands: scalar add / sub, bitwise ops, comparisons, min / max ----------------------------------------
    # A clear operand is one of three things.
    #   One Python int for the whole batch: the reference restated, its early-stop decomposers, the split into the
    #     blocks the scalar covers and the blocks compared with zero, the trivial results for a negative or an
    #     out-of-range scalar.  The DAG depends on the value; the digits are folded into block ops and LUT choices
    #     on the host.
    #   A numpy uint64 array of K values, one per row: checked against 2^T on the host, uploaded once per call.
    #   A torch int64 tensor of K values on the engine's device, read as u64: no copy and no check (values below
    #     2^T are the caller's promise); the form that a captured hipGraph serves with new values on every replay.
    # The per-row forms need T = bits * blocks <= 64 and run the full-width DAG: every block takes part, as if every
    # scalar had all its digits, and the digit of row r reaches the layer on the device (_PbsLayer.flush_clear).
    # What a row of a per-row result equals: for scalar_add / scalar_sub the one-int form called with that row's
    # scalar, bit for bit, always.  For the other operations bit for bit wherever the scalar's top message digit is
    # not 0 (the reference's DAG is then the full-width one: nothing is compared with zero, no block is left out),
    # and after decryption for smaller scalars.
    @staticmethod
    def _early_stop_digits(value: int, bits: int) -> list:
        """BlockDecomposer::with_early_stop_at_zero (block_decomposition.rs): the digits up to the last non-zero one"""
        out = []
        while value:
            out.append(value & ((1 << bits) - 1))
            value >>= bits
        return out

    def _scalar_refusal(self):
        if self.msg & (self.msg - 1):
            return "the message modulus is not a power of two: a clear operand is decomposed into whole bits"
        return None

    def _clear(self, name: str, ct: RadixBatch, value, negative: bool = False):
        """The clear operand of `name`: a Python int, or _ClearRows for one value per row of ct."""
        T = self.bits * ct.num_blocks
        per_row = "one Python int, a numpy uint64 array or a torch int64 tensor on the engine's device, of one value per row"
        if isinstance(value, np.ndarray) or type(value).__module__.split(".")[0] == "torch":
            host = isinstance(value, np.ndarray)
            if str(value.dtype) not in (("uint64",) if host else ("torch.int64",)):
                raise TypeError(f"integer {name}: the clear operand is {per_row}, got dtype {value.dtype}")
            if tuple(value.shape) != (ct.count,):
                raise ValueError(f"integer {name}: {ct.count} rows against clear operands of shape {tuple(value.shape)}")
            self._require(name, None if T <= 64 else
                          f"one clear operand per row is one u64, and the ciphertexts hold {T} bits")
            if host:
                if T < 64 and (value >> np.uint64(T)).any():
                    raise ValueError(f"integer {name}: a clear operand per row must be below 2^{T}, the ciphertexts' range")
                return _ClearRows(host=np.ascontiguousarray(value))
            if isinstance(self.ops, _DeviceOps) and (value.device != self.ops.device or not value.is_contiguous()):
                raise ValueError(f"integer {name}: the clear operands must be contiguous on {self.ops.device}, "
                                 f"got {value.device}")
            return _ClearRows(dev=value)
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise TypeError(f"integer {name}: the clear operand is {per_row}, got {type(value).__name__}")
        if value < 0 and not negative:
            raise ValueError(f"integer {name}: the clear operand must not be negative, got {value}")
        return int(value)

    def _family(self, key, functions) -> _LutFamily:
        """the family of the LUTs _lut(key + (s,), functions[s]), cached like them"""
        t = self._luts.get(("family",) + key)
        if t is None:
            t = self._luts[("family",) + key] = _LutFamily([self._lut(key + (s,), f) for s, f in enumerate(functions)])
        return t

    # -- scalar add / sub -----------------------------------------------------------------------------------------------
    def _unchecked_scalar_add_assign(self, ct: RadixBatch, clear, negate: bool):
        """unchecked_scalar_add_assign (radix/scalar_add.rs:53-65) and unchecked_scalar_sub_assign
        (radix/scalar_sub.rs:109-122): block j gets the digit of the scalar, or of its negation
        (create_negated_block_decomposer, scalar_sub.rs:68-107: the two's complement, padded with ones), times delta
        on its body (shortint unchecked_scalar_add_assign), and its degree grows by the digit.  No PBS, one
        block-layer call.  One value per row: one clear block-layer call over every block, and every degree grows
        by msg - 1, the largest digit, whatever the values are (numpy arrays included: the DAG that follows must
        not depend on them)."""
        nb, bits, delta = ct.num_blocks, self.bits, self.p.delta
        if isinstance(clear, _ClearRows):
            self.ops.clear_block_layer([
                (self.ops.block(ct, j), 0, [(self.ops.block(ct, j), 1)],
                 dict(rows=clear, negate=int(negate), shift=j * bits, bits=bits, scale=delta, index=None, lut_base=0))
                for j in range(nb)])
            ct.degree = [d + self.msg - 1 for d in ct.degree]
            return
        if negate:
            digits = [((-clear) >> (j * bits)) & (self.msg - 1) for j in range(nb)] if clear else []
        else:
            digits = self._early_stop_digits(clear, bits)[:nb]
        self.ops.block_layer([(self.ops.block(ct, j), d * delta, [(self.ops.block(ct, j), 1)])
                              for j, d in enumerate(digits) if d])
        for j, d in enumerate(digits):
            ct.degree[j] += d

    def _scalar_add(self, op: str, ct: RadixBatch, scalar, unchecked: bool, assign: bool):
        """{unchecked_,}scalar_{add,sub}[_assign]: the default forms (radix_parallel/scalar_add.rs:249-265,
        scalar_sub.rs:99-115) propagate a dirty operand first and the single carries afterwards; the assign forms
        take a resident operand."""
        name = (f"unchecked_scalar_{op}" + ("_assign" if assign else "") if unchecked else
                f"scalar_{op}" + ("_assign" if assign else "") + "_parallelized")
        clear = self._clear(name, ct, scalar)
        self._require(name, self._scalar_refusal() or (None if unchecked else self.propagation_refusal))
        res = ct if assign else self._resident(ct).clone()
        if not unchecked and not res.block_carries_are_empty(self.msg):
            self.full_propagate(res)
        self._unchecked_scalar_add_assign(res, clear, op == "sub")
        if not unchecked:
            self._propagate_single_carry_low_latency(res)
        return None if assign else res

    # -- scalar bitwise ops ---------------------------------------------------------------------------------------------
    def _scalar_bitop(self, op: str, lhs: RadixBatch, scalar, unchecked: bool, assign: bool):
        """{unchecked_,}scalar_bit{and,or,xor}[_assign]_parallelized (radix_parallel/scalar_bitwise_op.rs:17-45,
        127-136, 148-170, 273-295) over shortint unchecked_scalar_bit*_assign (shortint scalar_bitwise_op.rs:50, 110,
        169: the LUT x -> (x % msg op s) % msg): one PBS per block the scalar's digits cover; beyond its last digit
        bitand leaves trivial zeros and the other two leave the blocks as they are.  One value per row: every block,
        with the family of the msg LUTs of a digit; its degree is the largest of the family's, msg - 1."""
        name = ("unchecked_" if unchecked else "") + f"scalar_{op}" + ("_assign" if assign else "") + "_parallelized"
        clear = self._clear(name, lhs, scalar)
        self._require(name, self._scalar_refusal())
        res = lhs if assign else self._resident(lhs).clone()
        if not unchecked and not res.block_carries_are_empty(self.msg):
            self.full_propagate(res)
        f, m, nb, bits = self._BITOPS[op][0], self.msg, res.num_blocks, self.bits
        functions = [lambda x, s=s: f(x % m, s) % m for s in range(m)]
        layer = _PbsLayer(self)
        if isinstance(clear, _ClearRows):
            family = self._family((f"scalar_{op}",), functions)
            for j in range(nb):
                layer.add(res, j, family, clear=(clear, 0, j * bits, bits, 0))
            layer.flush()
        else:
            digits = self._early_stop_digits(clear, bits)[:nb]
            for j, s in enumerate(digits):
                layer.add(res, j, self._lut((f"scalar_{op}", s), functions[s]))
            layer.flush()
            if op == "bitand":
                for j in range(len(digits), nb):
                    self._set_trivial(res, j, 0)
        return None if assign else res

    # -- scalar eq / ne ---------------------------------------------------------------------------------------------------
    def _trivial_block(self, count: int, value: int) -> RadixBatch:
        """create_trivial / create_trivial_boolean_block: one trivial block holding `value` in every row"""
        rb = self.create_trivial_zero(count, 1)
        if value:
            self._set_trivial(rb, 0, value)
        return rb

    def _one_block(self, rb: RadixBatch, j: int) -> RadixBatch:
        """block j of rb as a batch of its own"""
        if rb.num_blocks == 1:
            return rb
        out = self._new(rb.count, 1)
        self.ops.block_layer([(self.ops.block(out, 0), 0, [(self.ops.block(rb, j), 1)])])
        out.degree, out.noise = [rb.degree[j]], [rb.noise[j]]
        return out

    def _packed(self, lhs: RadixBatch, chunk: list) -> list:
        """pack_block_chunk (scalar_comparison.rs:104-138) as prepare terms: msg * high + low, or the one block"""
        return [(lhs, chunk[1], self.msg), (lhs, chunk[0], 1)] if len(chunk) == 2 else [(lhs, chunk[0], 1)]

    def _unchecked_scalar_equality(self, op: str, lhs: RadixBatch, clear) -> RadixBatch:
        """unchecked_scalar_{eq,ne}_parallelized (scalar_comparison.rs:366-558), unsigned: a negative scalar and one
        with a non-zero packed digit beyond the ciphertext give a trivial answer; pairs of blocks the scalar's packed
        digits cover are packed and compared with the digit by the LUT x -> x == s (create_scalar_comparison_luts,
        :312-336), the blocks above are compared with zero in the same pass (compare_blocks_with_zero), and the
        0 / 1 blocks are reduced (are_all_ / is_at_least_one_comparisons_block_true).  A packed digit is
        2 * log2(msg) bits, the reference's total_modulus.ilog2() where carry == msg.  One value per row: every
        pair, with the family of the msg^2 LUTs of a packed digit; an odd last block takes the digits below msg of
        the same family."""
        eq, m, nb, K, pbits = op == "eq", self.msg, lhs.num_blocks, lhs.count, 2 * self.bits
        assert nb > 0 and lhs.block_carries_are_empty(m)
        compare = (lambda x, s: int(x == s)) if eq else (lambda x, s: int(x != s))
        functions = [lambda x, s=s: compare(x, s) for s in range(m * m)]
        chunks = [list(range(j, min(j + 2, nb))) for j in range(0, nb, 2)]
        layer = _PbsLayer(self)
        if isinstance(clear, _ClearRows):
            family = self._family((f"scalar_{op}",), functions)
            out = self._new(K, len(chunks))
            for c, chunk in enumerate(chunks):
                layer.add(out, c, family, prepare=(0, self._packed(lhs, chunk)),
                          clear=(clear, 0, c * pbits, pbits if len(chunk) == 2 else self.bits, 0))
            layer.flush()
            blocks = [(out, c) for c in range(len(chunks))]
        else:
            if clear < 0:
                return self._trivial_block(K, int(not eq))
            digits = self._early_stop_digits(clear, pbits)
            if any(digits[len(chunks):]):                     # is_scalar_obviously_bigger
                return self._trivial_block(K, int(not eq))
            digits = digits[:len(chunks)]
            split = min(nb, 2 * len(digits))

            def covered():
                if not digits:
                    return []
                out = self._new(K, len(digits))
                for c, s in enumerate(digits):
                    layer.add(out, c, self._lut((f"scalar_{op}", s), functions[s]), prepare=(0, self._packed(lhs, chunks[c])))
                yield
                return [(out, c) for c in range(len(digits))]

            low, high = self._join(layer, covered(), self._compare_blocks_with_zero_steps(
                layer, [(lhs, j) for j in range(split, nb)], eq))
            blocks = low + high
        (res,) = self._join(layer, self._comparisons_block_true_steps(layer, K, blocks, eq))
        return self._one_block(*res)

    # -- scalar order -----------------------------------------------------------------------------------------------------
    def _reduce_signs_steps(self, layer: _PbsLayer, count: int, blocks: list):
        """reduce_signs_parallelized (comparator.rs:257-280) as a branch of _join: pairs 4 * high + low through
        comparison_reduction_lut until one sign is left"""
        table = [IS_INFERIOR] * 5 + [IS_EQUAL] + [IS_SUPERIOR] * 5
        reduction = self._lut(("sign_reduction",), lambda x: table[x] if x < len(table) else 0)
        while len(blocks) != 1:
            out = self._new(count, len(blocks) // 2)
            for c in range(len(blocks) // 2):
                (low, lj), (high, hj) = blocks[2 * c], blocks[2 * c + 1]
                layer.add(out, c, reduction, prepare=(0, [(high, hj, 4), (low, lj, 1)]))
            yield
            blocks = [(out, c) for c in range(len(blocks) // 2)] + (blocks[-1:] if len(blocks) % 2 else [])
        return blocks[0]

    def _unchecked_scalar_compare(self, lhs: RadixBatch, clear):
        """unsigned_unchecked_scalar_compare_blocks_parallelized (comparator.rs:677-783): the sign (batch, block) of
        lhs against the scalar.  The blocks the scalar's digits cover are packed in pairs, the packed digit times
        delta is subtracted on the body, sign_lut, + 1 (scalar_compare_block_assign, :226-238), and the signs are
        reduced; the blocks above are compared with zero, reduced, and mapped to IS_EQUAL / IS_SUPERIOR; both
        branches share their passes (rayon::join), and one more reduction joins the two signs.  One value per row:
        every pair, the packed digit of row r times -delta from the clear block layer."""
        m, nb, K, bits, delta = self.msg, lhs.num_blocks, lhs.count, self.bits, self.p.delta
        assert nb > 0 and lhs.block_carries_are_empty(m)
        sign_lut = self._lut(("sign",), lambda x: int(x != 0))
        layer = _PbsLayer(self)
        if isinstance(clear, _ClearRows):
            chunks = [list(range(j, min(j + 2, nb))) for j in range(0, nb, 2)]
            signs = self._new(K, len(chunks))
            for c, chunk in enumerate(chunks):
                layer.add(signs, c, sign_lut, prepare=(0, self._packed(lhs, chunk)), post_add=1,
                          clear=(clear, 0, c * 2 * bits, len(chunk) * bits, -delta))
            layer.flush()
            (sign,) = self._join(layer, self._reduce_signs_steps(layer, K, [(signs, c) for c in range(len(chunks))]))
            return sign
        if clear < 0:
            return self._trivial_block(K, IS_SUPERIOR), 0
        digits = self._early_stop_digits(clear, bits)
        if any(digits[nb:]):                                  # is_scalar_obviously_bigger
            return self._trivial_block(K, IS_INFERIOR), 0
        digits = digits[:nb]

        def covered():
            chunks = [list(range(j, min(j + 2, len(digits)))) for j in range(0, len(digits), 2)]
            signs = self._new(K, len(chunks))
            for c, chunk in enumerate(chunks):
                packed = sum(digits[j] * m ** i for i, j in enumerate(chunk))
                layer.add(signs, c, sign_lut, prepare=(-packed * delta, self._packed(lhs, chunk)), post_add=1)
            yield
            return (yield from self._reduce_signs_steps(layer, K, [(signs, c) for c in range(len(chunks))]))

        def above():
            zero = yield from self._compare_blocks_with_zero_steps(layer, [(lhs, j) for j in range(len(digits), nb)], True)
            rb, j = yield from self._comparisons_block_true_steps(layer, K, zero, True)
            out = self._new(K, 1)
            layer.add(out, 0, self._lut(("sign_of_upper_zero",), lambda x: IS_EQUAL if x == 1 else IS_SUPERIOR),
                      prepare=(0, [(rb, j, 1)]))
            yield
            return out, 0

        signs = self._join(layer, *([covered()] if digits else []), *([above()] if len(digits) < nb else []))
        if len(signs) == 1:
            return signs[0]
        (low, lj), (high, hj) = signs                         # reduce_two_sign_blocks_assign(msb_sign, lsb_sign)
        (sign,) = self._join(layer, self._reduce_signs_steps(layer, K, [(low, lj), (high, hj)]))
        return sign

    def _trivial_radix(self, count: int, nb: int, clear) -> RadixBatch:
        """create_trivial_radix (radix/mod.rs): the digits of the scalar modulo 2^T as trivial blocks, of the
        digit's degree.  One value per row: one clear block-layer call of term-less ops (a zero mask, the digit
        times delta on the body), degree msg - 1."""
        if isinstance(clear, _ClearRows):
            rb = self._new(count, nb)
            self.ops.clear_block_layer([
                (self.ops.block(rb, j), 0, [], dict(rows=clear, negate=0, shift=j * self.bits, bits=self.bits,
                                                    scale=self.p.delta, index=None, lut_base=0)) for j in range(nb)])
            rb.degree = [self.msg - 1] * nb
            return rb
        rb = self.create_trivial_zero(count, nb)
        for j in range(nb):
            digit = (clear >> (j * self.bits)) & (self.msg - 1)
            if digit:
                self._set_trivial(rb, j, digit)
        return rb

    def _scalar_comparison(self, op: str, lhs: RadixBatch, scalar, unchecked: bool) -> RadixBatch:
        """{unchecked_,}scalar_{eq,ne,gt,ge,lt,le,max,min}_parallelized (scalar_comparison.rs:366-680,
        comparator.rs:877-912, 1468-1535, 1618-1710): the default forms work on a propagated clone of a dirty
        operand.  eq / ne need carry >= msg, as the reference asserts (:399); the order comparisons pack as well."""
        name = ("unchecked_" if unchecked else "") + f"scalar_{op}_parallelized"
        clear = self._clear(name, lhs, scalar, negative=True)
        refusal = self.bivariate_refusal if op in ("eq", "ne") else (self.comparison_refusal or self.bivariate_refusal)
        self._require(name, self._scalar_refusal() or refusal)
        lhs = self._resident(lhs) if unchecked else self._clean(lhs)
        if op in ("eq", "ne"):
            return self._unchecked_scalar_equality(op, lhs, clear)
        sign, sj = self._unchecked_scalar_compare(lhs, clear)
        if op in self._ORDER:                                 # map_sign_result (comparator.rs:957-971)
            res = self._new(lhs.count, 1)
            layer = _PbsLayer(self)
            layer.add(res, 0, self._lut(("sign_is", op), lambda x, f=self._ORDER[op]: int(f(x))),
                      prepare=(0, [(sign, sj, 1)]))
            layer.flush()
            return res
        keep = IS_SUPERIOR if op == "max" else IS_INFERIOR    # unchecked_scalar_min_or_max_parallelized
        rhs = self._trivial_radix(lhs.count, lhs.num_blocks, clear)
        return self._programmable_if_then_else(sign, sj, lhs, rhs, op, lambda x: x == keep)

    # ---- shifts and rotations by a clear amount, by an encrypted amount, scalar_mul -------------------------------
    # Every PBS layer is a fused _PbsLayer again.  A block rotation is never a data movement: it is the source block
    # index of the prepare terms, and the outputs are scattered into a fresh batch, so no op of a block-layer call
    # reads a block another op of the same call writes.  A clear operand is one non-negative Python int for the
    # whole batch: the DAG depends on its value.
    _SHIFTS = ("left_shift", "right_shift", "rotate_left", "rotate_right")

    @staticmethod
    def _clear_operand(op: str, value) -> int:
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise TypeError(f"integer {op}: the clear operand is one Python int for the whole batch, "
                            f"got {type(value).__name__}")
        if value < 0:
            raise ValueError(f"integer {op}: the clear operand must not be negative, got {value}")
        return int(value)

    @staticmethod
    def _assign(ct: RadixBatch, res: RadixBatch):
        if res is not ct:
            ct.data, ct.degree, ct.noise = res.data, list(res.degree), list(res.noise)

    def _scalar_shift_luts(self, op: str, within: int):
        """(LUT of a window, LUT of a shift's end block) for a shift of `within` bits inside the blocks.
        left_shift (scalar_shift.rs:603-615) packs previous * msg + current, the other three pack the block that
        stays * msg + the neighbour that gives bits: right_shift (:342-357) current * msg + next, the rotations
        (scalar_rotate.rs:309-324, 644-654) receiver * msg + giver.  The end block of a shift takes shortint
        scalar_left_shift_assign / scalar_right_shift_assign (shortint/server_key/shift.rs:411-415, 145-148)."""
        m, bits, w = self.msg, self.bits, within
        if op == "left_shift":
            window = lambda previous, current: ((current << w) % m) + ((previous << w) // m)
            end = self._lut((op, w, "end"), lambda x: (x << w) % m)
        elif op == "rotate_left":
            window, end = (lambda receiver, giver: ((receiver << w) % m) + ((giver << w) // m)), None
        else:
            window = lambda current, giver: (current >> w) + (((giver << bits) >> w) % m)
            end = self._lut((op, w, "end"), lambda x: ((x % m) >> w) % m) if op == "right_shift" else None
        return self._lut((op, w), window, bivariate=True), end

    def _scalar_shift_queue(self, layer: _PbsLayer, ct: RadixBatch, op: str, amount: int) -> RadixBatch:
        """unchecked_scalar_{left,right}_shift_assign_parallelized (scalar_shift.rs:553-647, 246-368) and
        unchecked_scalar_rotate_{left,right}_assign_parallelized (scalar_rotate.rs:611-681, 272-350) into a fresh
        batch; the PBS requests are queued on `layer` (the caller flushes it: scalar_mul shares one layer among its
        preshifts).  amount mod T == 0 returns ct itself.  Result block j reads block j -+ rotations of ct: the
        blocks a shift vacates are trivial zeros.  With nothing to shift inside the blocks there is no PBS: one
        block-layer call copies the blocks to their places."""
        nb, bits, m = ct.num_blocks, self.bits, self.msg
        assert nb > 0 and ct.block_carries_are_empty(m)
        amount %= bits * nb
        if amount == 0:
            return ct
        rot, within = divmod(amount, bits)
        left, shift = op in ("left_shift", "rotate_left"), op in ("left_shift", "right_shift")
        step = -rot if left else rot                  # rotate_right(rot) of the blocks for the left forms

        def source(j):
            """the block of ct that stands at place j after the block rotation; None: a vacated place"""
            i = j + step
            return i % nb if not shift or 0 <= i < nb else None

        if within == 0:
            res = self._new(ct.count, nb)
            moves = []
            for j in range(nb):
                i = source(j)
                moves.append((self.ops.block(res, j), 0, [] if i is None else [(self.ops.block(ct, i), 1)]))
                if i is not None:
                    res.degree[j], res.noise[j] = ct.degree[i], ct.noise[i]
            self.ops.block_layer(moves)
            return res
        window, end = self._scalar_shift_luts(op, within)
        res = self.create_trivial_zero(ct.count, nb) if shift and rot else self._new(ct.count, nb)
        giver = -1 if left else 1                     # the neighbour a place takes bits from
        for j in range(nb):
            i = source(j)
            g = source(j + giver) if not shift or 0 <= j + giver < nb else None
            if i is None:
                continue
            if g is None:                             # the end block of a shift pulls in zeros
                layer.add(res, j, end, prepare=(0, [(ct, i, 1)]))
            elif op == "left_shift":
                layer.add(res, j, window, prepare=(0, [(ct, g, m), (ct, i, 1)]))
            else:
                layer.add(res, j, window, prepare=(0, [(ct, i, m), (ct, g, 1)]))
        return res

    def _unchecked_scalar_shift(self, op: str, ct: RadixBatch, amount, assign: bool = False) -> RadixBatch:
        name = f"unchecked_scalar_{op}{'_assign' if assign else ''}_parallelized"
        amount = self._clear_operand(name, amount)
        self._require(name, self.bivariate_refusal)
        layer = _PbsLayer(self)
        res = self._scalar_shift_queue(layer, self._resident(ct), op, amount)
        layer.flush()
        return res

    def _scalar_shift(self, op: str, ct: RadixBatch, amount, assign: bool) -> RadixBatch:
        """scalar_{left_shift,right_shift,rotate_left,rotate_right}[_assign]_parallelized (scalar_shift.rs:451-461,
        732-742, scalar_rotate.rs): full_propagate first when the operand has carries, on the operand itself in
        the assign form and on a clone otherwise."""
        name = f"scalar_{op}{'_assign' if assign else ''}_parallelized"
        amount = self._clear_operand(name, amount)
        self._require(name, self.bivariate_refusal)
        if not assign:
            return self._unchecked_scalar_shift(op, self._clean(ct), amount)
        if not ct.block_carries_are_empty(self.msg):
            self.full_propagate(ct)
        self._assign(ct, self._unchecked_scalar_shift(op, ct, amount))
        return ct

    # -- encrypted amount -------------------------------------------------------------------------------------------
    def _barrel_shifter(self, ct: RadixBatch, shift: RadixBatch, operation: str) -> RadixBatch:
        """barrel_shifter (radix_parallel/shift.rs:321-473) into a fresh batch.  Layer 1 extracts every bit of ct
        (BitExtractor, bit_extractor.rs:52-67) and the first s bits of shift, born at bit 2
        (with_final_offset(.., 2)); the reference joins the two extractions.  One layer per control bit d follows:
        bit i becomes mux_lut(2 * b + a + control_d), a = bit i, b = bit i -+ 2^d (mod T, or the padding -- a
        trivial zero, so no term -- where a shift pulls it in); a stage reads the bits of the stage before and
        writes a fresh batch.  The last layer recomposes sum_i 2^i * bit_i per block under lut_message."""
        nb, bits = ct.num_blocks, self.bits
        assert ct.block_carries_are_empty(self.msg) and shift.block_carries_are_empty(self.msg)
        T = bits * nb
        s = T.bit_length() - 1 + (1 if T & (T - 1) else 0)          # shift.rs:345-353
        K = ct.count
        a, control = self._new(K, T), self._new(K, s)
        layer = _PbsLayer(self)
        for n in range(T):
            layer.add(a, n, self._lut(("bit", n % bits, 0), lambda x, i=n % bits: (x >> i) & 1),
                      prepare=(0, [(ct, n // bits, 1)]))
        for n in range(s):
            layer.add(control, n, self._lut(("bit", n % bits, 2), lambda x, i=n % bits: ((x >> i) & 1) << 2),
                      prepare=(0, [(shift, n // bits, 1)]))
        layer.flush()
        mux = self._lut(("mux",), lambda x: (x >> 1) & 1 if (x >> 2) & 1 else x & 1)
        left, rotate = operation in ("left_shift", "rotate_left"), operation in ("rotate_left", "rotate_right")
        for d in range(s):
            out = self._new(K, T)
            for i in range(T):
                b = i - (1 << d) if left else i + (1 << d)
                terms = [(a, b % T, 2)] if rotate or 0 <= b < T else []
                assert 2 * 1 + a.degree[i] + control.degree[d] < self.msg * self.carry      # control | b | a
                layer.add(out, i, mux, prepare=(0, terms + [(a, i, 1), (control, d, 1)]))
            layer.flush()
            a = out
        res = self._new(K, nb)
        for j in range(nb):
            layer.add(res, j, self.lut_message, prepare=(0, [(a, j * bits + i, 1 << i) for i in range(bits)]))
        layer.flush()
        return res

    def _encrypted_shift(self, op: str, ct: RadixBatch, shift: RadixBatch, unchecked: bool, assign: bool) -> RadixBatch:
        """{unchecked_,}{left_shift,right_shift,rotate_left,rotate_right}[_assign]_parallelized (shift.rs:20-298,
        rotate.rs).  The default forms propagate whichever operand has carries: shift on a clone, ct itself in the
        assign form and on a clone otherwise.  The reference takes the block count of shift for both operands and
        panics on its closing assert when they differ (shift.rs:329, 457): a ValueError here."""
        name = f"{'unchecked_' if unchecked else ''}{op}{'_assign' if assign else ''}_parallelized"
        self._require(name, self.barrel_shifter_refusal)
        if ct.num_blocks != shift.num_blocks or ct.num_blocks == 0:
            raise ValueError(f"integer {name}: the value has {ct.num_blocks} blocks and the amount {shift.num_blocks}; "
                             "the barrel shifter takes operands of the same, non-zero block count")
        if ct.count != shift.count:
            raise ValueError(f"integer {name}: {ct.count} values against {shift.count} amounts")
        if unchecked:
            ct_in, shift = self._resident(ct), self._resident(shift)
        else:
            shift = self._clean(shift)
            if assign and not ct.block_carries_are_empty(self.msg):
                self.full_propagate(ct)
            ct_in = self._clean(ct)
        res = self._barrel_shifter(ct_in, shift, op)
        if assign:
            self._assign(ct, res)
            return ct
        return res

    # -- scalar_mul ---------------------------------------------------------------------------------------------------
    def _require_scalar_mul(self, name: str, scalar: int):
        """0 and 1 need nothing, a power of two the shift's bivariate layer, the rest the chunked sum as well"""
        if scalar > 1:
            self._require(name, self.bivariate_refusal or (self.propagation_refusal if scalar & (scalar - 1) else None))

    def _unchecked_scalar_mul(self, name: str, ct: RadixBatch, scalar: int) -> RadixBatch:
        """unchecked_scalar_mul_assign_parallelized (radix_parallel/scalar_mul.rs:330-397) into a fresh batch (ct
        itself for scalar 1).  One deviation: a power of two 2^e with e >= T gives trivial zeros, the product
        modulo 2^T, where the reference shifts by e mod T (:346-350 over scalar_shift.rs:576)."""
        self._require_scalar_mul(name, scalar)
        ct = self._resident(ct)
        nb, bits = ct.num_blocks, self.bits
        if scalar == 0 or nb == 0:
            return self.create_trivial_zero(ct.count, nb)
        if scalar == 1:
            return ct
        if scalar & (scalar - 1) == 0:
            e = scalar.bit_length() - 1
            if e >= bits * nb:
                return self.create_trivial_zero(ct.count, nb)
            return self._unchecked_scalar_shift("left_shift", ct, e)
        scalar_bits = [(scalar >> i) & 1 for i in range(scalar.bit_length())]   # LSB first, up to the last set bit
        needed = {i % bits for i, bit in enumerate(scalar_bits) if bit}          # has_at_least_one_set
        layer = _PbsLayer(self)
        preshifted = {w: self._scalar_shift_queue(layer, ct, "left_shift", w) for w in sorted(needed)}
        layer.flush()                                    # the reference's par_iter over the shifts: one layer
        terms = [self.blockshift(preshifted[i % bits], i // bits)
                 for i, bit in enumerate(scalar_bits[:bits * nb]) if bit]
        out = self.unchecked_sum_ciphertexts_vec(terms)
        return out if out is not None else self.create_trivial_zero(ct.count, nb)

    def unchecked_scalar_mul_parallelized(self, ct: RadixBatch, scalar) -> RadixBatch:
        name = "unchecked_scalar_mul_parallelized"
        return self._unchecked_scalar_mul(name, ct, self._clear_operand(name, scalar))

    def unchecked_scalar_mul_assign_parallelized(self, ct: RadixBatch, scalar):
        name = "unchecked_scalar_mul_assign_parallelized"
        self._assign(ct, self._unchecked_scalar_mul(name, ct, self._clear_operand(name, scalar)))

    def scalar_mul_parallelized(self, ct: RadixBatch, scalar) -> RadixBatch:
        """scalar_mul.rs:483-491."""
        name = "scalar_mul_parallelized"
        scalar = self._clear_operand(name, scalar)
        self._require_scalar_mul(name, scalar)
        return self._unchecked_scalar_mul(name, self._clean(ct), scalar)

    def scalar_mul_assign_parallelized(self, ct: RadixBatch, scalar):
        """scalar_mul.rs:493-503."""
        name = "scalar_mul_assign_parallelized"
        scalar = self._clear_operand(name, scalar)
        self._require_scalar_mul(name, scalar)
        if not ct.block_carries_are_empty(self.msg):
            self.full_propagate(ct)
        self._assign(ct, self._unchecked_scalar_mul(name, ct, scalar))

    # ---- overflowing sub, zero tests, division ------------------------------------------------------------------------
    # The deepest DAGs of the layer: a division is bits * blocks dependent iterations.  Every PBS layer is a fused
    # _PbsLayer, and nothing runs between two layers: a radix value is a list of (batch, block) here, so a slice, a
    # rotation, a prepended block or the carry-over of a prefix-sum step is a list operation, every sum or difference
    # of blocks is the prepare op of the request that consumes it, and every output goes to a fresh batch (no op of a
    # block-layer call reads what another writes).  Branches the reference joins run in lockstep through _join and
    # share their passes.  On the device the tables come from one _LayerPlan per operand shape (_DeviceOps.plan).
    @staticmethod
    def _terms(blocks, scalar: int = 1) -> list:
        return [(rb, j, scalar) for rb, j in blocks]

    @staticmethod
    def _shape_key(*operands) -> tuple:
        return tuple((rb.count, tuple(rb.degree), tuple(rb.noise)) for rb in operands)

    def _check_pair(self, name: str, lhs: RadixBatch, rhs: RadixBatch, what=("left", "right")):
        if lhs.num_blocks != rhs.num_blocks or lhs.num_blocks == 0:
            raise ValueError(f"integer {name}: the {what[0]} operand has {lhs.num_blocks} blocks and the {what[1]} one "
                             f"{rhs.num_blocks}; the operands take the same, non-zero block count")
        if lhs.count != rhs.count:
            raise ValueError(f"integer {name}: {lhs.count} {what[0]} operands against {rhs.count} {what[1]} ones")

    def _check_clean(self, name: str, *operands):
        if not all(rb.block_carries_are_empty(self.msg) for rb in operands):
            raise ValueError(f"integer {name}: the unchecked form takes operands with empty carries")

    # -- overflowing sub ------------------------------------------------------------------------------------------------
    def _borrow_luts(self):
        """generate_init_borrow_array's two LUTs (sub.rs:687-705): the first block generates a borrow or not, the
        others may also propagate one"""
        m = self.msg
        return (self._lut(("borrow_init", "first"), lambda x: BORROW_GENERATED if x < m else BORROW_NONE),
                self._lut(("borrow_init",), lambda x: BORROW_GENERATED if x < m else
                          (BORROW_PROPAGATED if x == m else BORROW_NONE)))

    def _overflowing_sub_steps(self, layer: _PbsLayer, count: int, lhs: list, rhs: list):
        """unchecked_unsigned_overflowing_sub_parallelized (sub.rs:355-421) as a branch of _join.  lhs: per block
        the [(batch, block)] whose sum is the block (the division hands remainder1 + remainder2 over unsummed); rhs:
        [(batch, block)].  Returns ([(batch, block)] of the difference, (batch, 0) of the output borrow, a one-block
        batch of degree 1).

        Block j of shortint unchecked_sub is lhs_j - rhs_j + z * delta, z = max(ceil(degree(rhs_j) / msg), 1) * msg
        (neg.rs:223-246): in msg .. 2 msg - 1 where the block needs no borrow, below msg where it does.  It is never
        stored: it is the prepare op of generate_init_borrow_array's LUT and, with the input borrow subtracted as a
        fourth term (the true LWE subtraction of sub.rs:410-414), of the closing message_extract.  The prefix sum
        (compute_borrow_propagation_parallelized_low_latency, sub.rs:727-765, over compute_prefix_sum_hillis_steele,
        add.rs:572-603) packs state_b * msg + state_(b - space) in the prepare op of its LUT and writes a fresh batch
        per step; a state that a step does not touch stays where it is.  The top state has a batch of its own in every
        step, so the output borrow is a whole batch."""
        m, nb, delta, total = self.msg, len(rhs), self.p.delta, self.msg * self.carry
        assert nb > 0 and len(lhs) == nb

        def difference(j, extra=()):
            z = max(-(-rhs[j][0].degree[rhs[j][1]] // m), 1) * m
            if sum(rb.degree[i] for rb, i in lhs[j]) + z >= total:       # overflowing_sub_refusal: carry >= 2
                raise ValueError(f"unsigned_overflowing_sub: block {j} of the difference overflows the block")
            return z * delta, self._terms(lhs[j]) + [(rhs[j][0], rhs[j][1], -1)] + list(extra)

        def fresh(first, last):
            """places of the states first .. last (last: the top one, in a batch of its own)"""
            low = self._new(count, last - first) if last > first else None
            return [(low, b - first) for b in range(first, last)] + [(self._new(count, 1), 0)]

        first_lut, other_lut = self._borrow_luts()
        states = fresh(0, nb - 1)
        for b, (rb, j) in enumerate(states):
            layer.add(rb, j, first_lut if b == 0 else other_lut, prepare=difference(b))
        yield
        space = 1
        for _ in range((nb - 1).bit_length()):                           # ceil_ilog2(nb) steps
            step = states[:space] + fresh(space, nb - 1)
            for b in range(space, nb):
                (hi, hj), (lo, lj) = states[b], states[b - space]
                # overflowing_sub_refusal: the borrow states fit the message bits, two of them the block
                assert lo.degree[lj] + 1 <= m and hi.degree[hj] * m + lo.degree[lj] < total
                layer.add(*step[b], self.lut_prefix, prepare=(0, [(hi, hj, m), (lo, lj, 1)]))
            yield
            for rb, j in step[space:]:
                # the prefix of borrow states is a borrow state, though the LUT that made it has degree msg - 1: with
                # carry < msg that degree would not pack in the next step, the states do (the reference packs them
                # unchecked, bivariate_pbs.rs:167-182)
                rb.degree[j] = BORROW_PROPAGATED
            states, space = step, space * 2
        res = self._new(count, nb)
        for j in range(nb):          # block j takes the output borrow of block j - 1, block 0 a trivial zero: no term
            layer.add(res, j, self.lut_message, prepare=difference(j, self._terms(states[j - 1:j] if j else [], -1)))
        yield
        out, oj = states[nb - 1]
        out.degree[oj] = 1           # a boolean, though the LUT that made it has degree 2 (sub.rs:418-421)
        return [(res, j) for j in range(nb)], (out, oj)

    def unchecked_unsigned_overflowing_sub_parallelized(self, lhs: RadixBatch, rhs: RadixBatch):
        """sub.rs:355-381: (lhs - rhs modulo msg ** blocks, lhs < rhs as a one-block batch of degree 1)."""
        name = "unchecked_unsigned_overflowing_sub_parallelized"
        self._require(name, self.overflowing_sub_refusal)
        self._check_pair(name, lhs, rhs)
        self._check_clean(name, lhs, rhs)
        lhs, rhs = self._resident(lhs), self._resident(rhs)
        nb = lhs.num_blocks
        with self.ops.plan(("overflowing_sub",) + self._shape_key(lhs, rhs),
                           list(self._borrow_luts()) + [self.lut_prefix, self.lut_message]):
            layer = _PbsLayer(self)
            (res, (borrow, _)), = self._join(layer, self._overflowing_sub_steps(
                layer, lhs.count, [[(lhs, j)] for j in range(nb)], [(rhs, j) for j in range(nb)]))
        return res[0][0], borrow

    def unsigned_overflowing_sub_parallelized(self, lhs: RadixBatch, rhs: RadixBatch):
        """sub.rs:318-353."""
        name = "unsigned_overflowing_sub_parallelized"
        self._require(name, self.overflowing_sub_refusal)
        self._check_pair(name, lhs, rhs)
        return self.unchecked_unsigned_overflowing_sub_parallelized(self._clean(lhs), self._clean(rhs))

    # -- zero tests -----------------------------------------------------------------------------------------------------
    def _compare_blocks_with_zero_steps(self, layer: _PbsLayer, blocks: list, equality: bool):
        """compare_blocks_with_zero (scalar_comparison.rs:254-296) as a branch of _join: blocks with empty carries are
        summed in chunks of (msg * carry - 1) // (msg - 1), one LUT per chunk tells whether the sum is zero (equality)
        or not.  blocks: [(batch, block)]; returns [(batch, block)] of 0 / 1, empty for no blocks."""
        if not blocks:
            return []
        total = self.msg * self.carry
        assert all(rb.degree[j] < self.msg for rb, j in blocks)
        fill = (total - 1) // (self.msg - 1)
        chunks = [blocks[c:c + fill] for c in range(0, len(blocks), fill)]
        out = self._new(blocks[0][0].count, len(chunks))
        lut = self._lut(("sum_is_zero",), lambda x: int(x % total == 0)) if equality else \
            self._lut(("sum_non_zero",), lambda x: int(x != 0))
        for c, chunk in enumerate(chunks):
            layer.add(out, c, lut, prepare=(0, self._terms(chunk)))
        yield
        return [(out, c) for c in range(len(chunks))]

    def _comparisons_block_true_steps(self, layer: _PbsLayer, count: int, blocks: list, all_true: bool):
        """are_all_comparisons_block_true / is_at_least_one_comparisons_block_true (scalar_comparison.rs:147-233) as a
        branch of _join: no block gives a trivial 1, one block comes back as it is, without a PBS."""
        if not blocks:
            one = self.create_trivial_zero(count, 1)
            self.ops.block_layer([(self.ops.block(one, 0), self.p.delta, [])])
            one.degree[0] = 1
            return one, 0
        return (yield from self._reduce_block_comparisons_steps(layer, blocks, all_true))

    def _are_all_comparisons_block_true_steps(self, layer: _PbsLayer, count: int, blocks: list):
        return self._comparisons_block_true_steps(layer, count, blocks, True)

    def _is_at_least_one_comparisons_block_true_steps(self, layer: _PbsLayer, count: int, blocks: list):
        return self._comparisons_block_true_steps(layer, count, blocks, False)

    # -- division -------------------------------------------------------------------------------------------------------
    def _div_luts(self) -> dict:
        """Every LUT a division can ask for, by role, in a fixed order: the one stack of its table plan."""
        m, bits = self.msg, self.bits
        first, other = self._borrow_luts()
        window, end = self._scalar_shift_luts("left_shift", 1)
        luts = {"borrow_first": first, "borrow": other, "prefix": self.lut_prefix, "message": self.lut_message,
                "shift": window, "shift_end": end, "non_zero": self._lut(("sum_non_zero",), lambda x: int(x != 0))}
        for pos in range(bits - 1):       # the trims at bit pos of a block (div_mod.rs:209-269)
            keep, drop = (m - 1) >> (bits - (pos + 1)), ((m - 1) << (pos + 1)) & (m - 1)
            luts["keep", pos] = self._lut(("mask", keep), lambda x, k=keep: x & k)
            luts["drop", pos] = self._lut(("mask", drop), lambda x, k=drop: x & k)
        for factor in (2, 3):             # overflow_sum.degree + 1: without and with upper divisor blocks
            for name, zero_when in (("zero_unless_overflow", lambda s: s == 0), ("zero_if_overflow", lambda s: s != 0)):
                luts[name, factor] = self._lut(("div", name, factor), lambda block, s, z=zero_when: 0 if z(s) else block,
                                               factor=factor)
        for pos in range(bits):           # merge_overflow_flags_luts (div_mod.rs:167-173)
            luts["quotient_bit", pos] = self._lut(("div", "quotient_bit", pos),
                                                  lambda x, y, p=pos: int(x == 0 and y == 0) << p, bivariate=True)
        return luts

    def _unchecked_div_rem(self, numerator: RadixBatch, divisor: RadixBatch):
        """unsigned_unchecked_div_rem_parallelized (div_mod.rs:92-492): the long division, most significant bit
        first.  One iteration at live width L (the blocks of the remainder that can be non-zero) is
          one pass: the two trims of the divisor at the bit boundary and R << 1 of remainder1 (with the numerator
            block prepended: a list insert, the block is the source of the shift's first terms) and of remainder2;
          max(2 + ceil(log2 L), depth of the zero test) passes, joined: the overflowing sub of remainder1 + remainder2
            and the live divisor blocks, the zero test of the divisor's upper blocks, the cleaned merged remainder;
          one pass: the two conditional zero-outs, with factor = overflow_sum.degree + 1, and the quotient bit.
        A last pass cleans quotient and remainder.  Returns (quotient, remainder), fresh batches.

        Quotient block j is the sum of its bits' blocks (the reference adds each to the block as it is made); the
        sum is the prepare op of the block's closing message_extract.  The numerator block that has given its last
        bit is shifted once more and dropped, as in the reference, and its PBS counted."""
        K, nb, bits, m, total = numerator.count, numerator.num_blocks, self.bits, self.msg, self.msg * self.carry
        lut = self._div_luts()
        with self.ops.plan(("div_rem",) + self._shape_key(numerator, divisor), list(lut.values())):
            zero = self.create_trivial_zero(K, 1)
            remainder1, remainder2 = [(zero, 0)] * nb, [(zero, 0)] * nb
            numerator_block_stack = [(numerator, j) for j in range(nb)]
            quotient_bits = [[] for _ in range(nb)]
            layer = _PbsLayer(self)
            for i in reversed(range(bits * nb)):
                block_of_bit, pos_in_block = divmod(i, bits)
                msb_bit_set = bits * nb - 1 - i
                live = msb_bit_set // bits + 1                           # last_non_trivial_block + 1
                interesting_divisor = [(divisor, j) for j in range(live)]
                divisor_ms_blocks = [(divisor, j) for j in range((msb_bit_set + 1) // bits, nb)]
                # -- pass 1: trims and shifts
                if (msb_bit_set + 1) % bits:
                    pos, trimmed = msb_bit_set % bits, self._new(K, 2)
                    layer.add(trimmed, 0, lut["keep", pos], prepare=(0, self._terms(interesting_divisor[-1:])))
                    interesting_divisor[-1] = (trimmed, 0)
                    if divisor_ms_blocks:
                        layer.add(trimmed, 1, lut["drop", pos], prepare=(0, self._terms(divisor_ms_blocks[:1])))
                        divisor_ms_blocks[0] = (trimmed, 1)
                shifted = []
                for blocks in ([numerator_block_stack.pop()] + remainder1[:live], remainder2[:live]):
                    assert all(rb.degree[j] < m for rb, j in blocks)     # div_refusal: two messages fit a block
                    out = self._new(K, len(blocks))
                    layer.add(out, 0, lut["shift_end"], prepare=(0, self._terms(blocks[:1])))
                    for j in range(1, len(blocks)):                      # previous * msg + current
                        layer.add(out, j, lut["shift"],
                                  prepare=(0, self._terms(blocks[j - 1:j], m) + self._terms(blocks[j:j + 1])))
                    shifted.append([(out, j) for j in range(len(blocks))])
                layer.flush()
                if pos_in_block != 0:                                    # bits left in the numerator block
                    numerator_block_stack.append(shifted[0][0])
                merged = [[a, b] for a, b in zip(shifted[0][1:], shifted[1])]   # remainder1 + remainder2, unsummed

                # -- joined passes: overflowing sub | upper blocks of the divisor != 0 | clean merged remainder
                def check_divisor_upper_blocks():
                    if not divisor_ms_blocks:
                        return None                                      # a trivial zero: no term below
                    tmp = yield from self._compare_blocks_with_zero_steps(layer, divisor_ms_blocks, False)
                    return (yield from self._is_at_least_one_comparisons_block_true_steps(layer, K, tmp))

                def create_clean_version_of_merged_remainder():
                    out = self._new(K, live)
                    for j in range(live):
                        layer.add(out, j, lut["message"], prepare=(0, self._terms(merged[j])))
                    yield
                    return [(out, j) for j in range(live)]

                (new_remainder, overflowed), upper_non_zero, cleaned = self._join(
                    layer, self._overflowing_sub_steps(layer, K, merged, interesting_divisor),
                    check_divisor_upper_blocks(), create_clean_version_of_merged_remainder())
                # -- last pass: zero-outs and quotient bit
                flags = [overflowed] + ([upper_non_zero] if upper_non_zero else [])
                overflow_sum_degree = sum(rb.degree[j] for rb, j in flags)
                assert overflow_sum_degree <= 2
                factor = overflow_sum_degree + 1
                assert (m - 1) * factor + overflow_sum_degree < total   # div_refusal: the factor-3 packing
                kept1, kept2, bit = self._new(K, live), self._new(K, live), self._new(K, 1)
                for j in range(live):
                    layer.add(kept1, j, lut["zero_unless_overflow", factor],
                              prepare=(0, self._terms(cleaned[j:j + 1], factor) + self._terms(flags)))
                    layer.add(kept2, j, lut["zero_if_overflow", factor],
                              prepare=(0, self._terms(new_remainder[j:j + 1], factor) + self._terms(flags)))
                layer.add(bit, 0, lut["quotient_bit", pos_in_block],
                          prepare=(0, self._terms(flags[:1], m) + self._terms(flags[1:])))
                layer.flush()
                remainder1[:live] = [(kept1, j) for j in range(live)]
                remainder2[:live] = [(kept2, j) for j in range(live)]
                quotient_bits[block_of_bit].append((bit, 0))
            quotient, remainder = self._new(K, nb), self._new(K, nb)
            for j in range(nb):
                layer.add(remainder, j, lut["message"], prepare=(0, self._terms([remainder1[j], remainder2[j]])))
                layer.add(quotient, j, lut["message"], prepare=(0, self._terms(quotient_bits[j])))
            layer.flush()
        return quotient, remainder

    def _div_rem(self, name: str, numerator: RadixBatch, divisor: RadixBatch, unchecked: bool, assign: bool):
        """The preamble of every division entry point (div_mod.rs:597-631, 656-864): refusal and shape checks before
        the first launch; the default forms propagate whichever operand has carries, the divisor on a clone, the
        numerator itself in an _assign form and on a clone otherwise."""
        self._require(name, self.div_refusal)
        self._check_pair(name, numerator, divisor, ("numerator", "divisor"))
        if unchecked:
            self._check_clean(name, numerator, divisor)
            return self._unchecked_div_rem(self._resident(numerator), self._resident(divisor))
        divisor = self._clean(divisor)
        if assign and not numerator.block_carries_are_empty(self.msg):
            self.full_propagate(numerator)
        return self._unchecked_div_rem(self._clean(numerator), divisor)

    def unchecked_div_rem_parallelized(self, numerator: RadixBatch, divisor: RadixBatch):
        """div_mod.rs:92-492 (unsigned): (quotient, remainder); a zero divisor gives (2^T - 1, numerator)."""
        return self._div_rem("unchecked_div_rem_parallelized", numerator, divisor, True, False)

    def div_rem_parallelized(self, numerator: RadixBatch, divisor: RadixBatch):
        """div_mod.rs:597-631."""
        return self._div_rem("div_rem_parallelized", numerator, divisor, False, False)


def _add_div_methods():
    """the eight div / rem forms over div_rem (div_mod.rs:656-864)"""
    def form(which, unchecked, assign):
        def f(self, numerator, divisor):
            res = self._div_rem(f.__name__, numerator, divisor, unchecked, assign)[which]
            if not assign:
                return res
            self._assign(numerator, res)
        return f

    for which, op in enumerate(("div", "rem")):
        for unchecked in (True, False):
            for assign in (True, False):
                f = form(which, unchecked, assign)
                name = f"{'unchecked_' if unchecked else ''}{op}{'_assign' if assign else ''}_parallelized"
                f.__name__ = f.__qualname__ = name
                setattr(ServerKey, name, f)


def _add_shift_methods():
    """the public names of the sixteen scalar and the sixteen encrypted forms"""
    def scalar(op, unchecked, assign):
        if unchecked and assign:
            def f(self, ct, amount):
                self._assign(ct, self._unchecked_scalar_shift(op, ct, amount, True))
        elif unchecked:
            def f(self, ct, amount):
                return self._unchecked_scalar_shift(op, ct, amount)
        elif assign:
            def f(self, ct, amount):
                self._scalar_shift(op, ct, amount, True)
        else:
            def f(self, ct, amount):
                return self._scalar_shift(op, ct, amount, False)
        return f

    def encrypted(op, unchecked, assign):
        if assign:
            def f(self, ct, shift):
                self._encrypted_shift(op, ct, shift, unchecked, True)
        else:
            def f(self, ct, shift):
                return self._encrypted_shift(op, ct, shift, unchecked, False)
        return f

    for op in ServerKey._SHIFTS:
        for unchecked in (True, False):
            for assign in (True, False):
                tail = f"{op}{'_assign' if assign else ''}_parallelized"
                forms = ((f"scalar_{tail}", scalar(op, unchecked, assign)), (tail, encrypted(op, unchecked, assign)))
                for name, f in forms:
                    name = ("unchecked_" if unchecked else "") + name
                    f.__name__ = f.__qualname__ = name
                    setattr(ServerKey, name, f)


def _add_scalar_methods():
    """the public names of the clear-operand forms, as the reference has them: unchecked_scalar_{add,sub}[_assign]
    and scalar_{add,sub}[_assign]_parallelized; the four forms of scalar_bit{and,or,xor}; unchecked_ and default
    scalar_{eq,ne,gt,ge,lt,le,max,min}_parallelized"""
    def named(name, f):
        f.__name__ = f.__qualname__ = name
        setattr(ServerKey, name, f)

    def add(op, unchecked, assign):
        return lambda self, ct, scalar: self._scalar_add(op, ct, scalar, unchecked, assign)

    def bitop(op, unchecked, assign):
        return lambda self, ct, scalar: self._scalar_bitop(op, ct, scalar, unchecked, assign)

    def comparison(op, unchecked):
        return lambda self, ct, scalar: self._scalar_comparison(op, ct, scalar, unchecked)

    for assign in (False, True):
        tail = "_assign" if assign else ""
        for op in ("add", "sub"):
            named(f"unchecked_scalar_{op}{tail}", add(op, True, assign))
            named(f"scalar_{op}{tail}_parallelized", add(op, False, assign))
        for op in ServerKey._BITOPS:
            named(f"unchecked_scalar_{op}{tail}_parallelized", bitop(op, True, assign))
            named(f"scalar_{op}{tail}_parallelized", bitop(op, False, assign))
    for op in ("eq", "ne", "max", "min") + tuple(ServerKey._ORDER):
        named(f"unchecked_scalar_{op}_parallelized", comparison(op, True))
        named(f"scalar_{op}_parallelized", comparison(op, False))


_add_shift_methods()
_add_div_methods()
_add_scalar_methods()


# ---- integer WoP-PBS (integer/wopbs/mod.rs) ----------------------------------------------------------
_U64 = (1 << 64) - 1


def encode_radix(val: int, basis: int, nb_block: int) -> list:
    """The nb_block digits of val in a power-of-two basis, least significant first."""
    mask, power, out = basis - 1, 1, []
    for _ in range(nb_block):
        out.append((val & (mask * power)) // power)
        power *= basis
    return out


def encode_mix_radix(val: int, basis: list, modulus: int) -> list:
    """val read as fields of basis[i] bits, least significant first: each field gives its digit modulo
    `modulus`, and what it holds above the digit's bits is carried into the fields that follow."""
    log_mod = int(np.log2(modulus))
    out = []
    for bits in basis:
        digit = val % modulus
        out.append(digit)
        val -= digit
        carry = (val % (1 << bits)) >> log_mod
        val = (val >> bits) + carry
    return out


def decode_radix(val: list, basis: int) -> int:
    result, shift = 0, 1
    for v in val:
        result = (result + v * shift) & _U64
        shift = (shift * basis) & _U64
    return result


def split_value_according_to_bit_basis(value: int, basis: list) -> list:
    out = []
    for bits in basis:
        out.append(value & ((1 << bits) - 1))
        value >>= bits
    return out


def _ceil_log2(x: int) -> int:
    return (x - 1).bit_length()


class WopbsKey:
    """integer WopbsKey (integer/wopbs/mod.rs) on RadixBatch: K integers share one degree vector, so their
    bit extractions and the composed call are batched over K.

    Execution.  Blocks are taken most significant first; blocks with the same number of bits go through
    ONE extract_bits call; the bits are concatenated to [K][total_bits][n+1] and ONE composed call follows
    (circuit bootstrap + vertical packing) with as many outputs as the LUT has, under one set of GGSWs.
    Host arrays are the path: a device-resident batch is brought to the host and the result returned in
    the residency it came in.  The engines are only reached through extract_bits,
    circuit_bootstrap_vertical_packing, keyswitch_with_key, keyswitch and the PBS calls."""

    def __init__(self, wopbs_key: ShortintWopbsKey):
        self.wopbs_key = wopbs_key

    @staticmethod
    def _shortint(key):
        """the shortint key inside an integer ClientKey / ServerKey (or the shortint key itself)."""
        return getattr(key, "key", None) or getattr(key, "shortint", None) or key

    @classmethod
    def new_wopbs_key(cls, cks, sks, parameters, device: int = 0, engine=None) -> "WopbsKey":
        return cls(ShortintWopbsKey.new_wopbs_key(cls._shortint(cks), cls._shortint(sks), parameters, device, engine))

    @classmethod
    def new_from_shortint(cls, wopbs_key: ShortintWopbsKey) -> "WopbsKey":
        return cls(wopbs_key)

    @classmethod
    def new_wopbs_key_only_for_wopbs(cls, cks, sks) -> "WopbsKey":
        return cls(ShortintWopbsKey.new_wopbs_key_only_for_wopbs(cls._shortint(cks), cls._shortint(sks)))

    @property
    def param(self):
        return self.wopbs_key.param

    # -- residency ---------------------------------------------------------------------------
    @staticmethod
    def _host(rb: RadixBatch):
        """(host u64 array, function putting a host array back where rb's data lives)."""
        if isinstance(rb.data, np.ndarray):
            return np.ascontiguousarray(rb.data, dtype=np.uint64), lambda a: a
        import torch

        dev = rb.data.device
        return (rb.data.cpu().numpy().view(np.uint64),
                lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev))

    # -- lookup tables -------------------------------------------------------------------------
    def _lut_size(self, total_bit: int) -> int:
        return max(self.param.polynomial_size, 1 << total_bit)

    def _delta(self) -> int:
        return (1 << 63) // (self.param.message_modulus * self.param.carry_modulus)

    def generate_lut_radix(self, ct: RadixBatch, f) -> np.ndarray:
        """integer/wopbs/mod.rs:523-565: [blocks][max(N, 2^total_bit)], block j indexed through
        ceil(log2(degree_j + 1)) bits, one bit of padding."""
        basis = self.param.message_modulus
        nb = ct.num_blocks
        deg_bits = [_ceil_log2(d + 1) for d in ct.degree]
        total_bit, modulus, delta = sum(deg_bits), basis ** nb, self._delta()
        lut = np.zeros((nb, self._lut_size(total_bit)), dtype=np.uint64)
        for idx in range(1 << total_bit):
            value = decode_radix(encode_mix_radix(idx, deg_bits, basis), basis)
            f_val = int(f(value % modulus)) % modulus
            for o, digit in enumerate(encode_radix(f_val, basis, nb)):
                lut[o, idx] = np.uint64((digit * delta) & _U64)
        return lut

    def generate_lut_radix_without_padding(self, ct: RadixBatch, f) -> np.ndarray:
        """integer/wopbs/mod.rs:593-629: every block indexed through all log2(message carry) bits; the carry
        bits of a block fold onto the message bits of the next."""
        p = self.param
        log_msg, log_carry = int(np.log2(p.message_modulus)), int(np.log2(p.carry_modulus))
        log_basis = log_msg + log_carry
        nb = ct.num_blocks
        size = self._lut_size(nb * log_basis)
        lut = np.zeros((nb, size), dtype=np.uint64)
        for index in range(size):
            value, rest = 0, index
            for i in range(nb):
                field = rest % (1 << (log_basis * (i + 1)))
                rest -= field
                value += field >> (log_carry * i)
            f_val = int(f(value))
            for o in range(nb):
                lut[o, index] = np.uint64((((f_val >> (log_carry * o)) % (1 << log_msg)) << (64 - log_basis)) & _U64)
        return lut

    def generate_lut_bivariate_radix(self, ct1: RadixBatch, ct2: RadixBatch, f) -> np.ndarray:
        """integer/wopbs/mod.rs:784-844: the index's low bits are ct1's, the bits above ct2's."""
        basis = self.param.message_modulus
        nb = ct1.num_blocks
        deg_bits = [[_ceil_log2(d + 1) for d in ct.degree] for ct in (ct1, ct2)]
        nbits = [sum(b) for b in deg_bits]
        modulus, delta = basis ** ct2.num_blocks, self._delta()
        lut = np.zeros((nb, self._lut_size(sum(nbits))), dtype=np.uint64)
        for idx in range(1 << sum(nbits)):
            split = (idx % (1 << nbits[0]), idx >> nbits[0])
            x, y = (decode_radix(encode_mix_radix(split[i], deg_bits[i], basis), basis) for i in range(2))
            f_val = int(f(x % modulus, y % modulus)) % modulus
            for o, digit in enumerate(encode_radix(f_val, basis, nb)):
                lut[o, idx] = np.uint64((digit * delta) & _U64)
        return lut

    # -- the WoP-PBS ---------------------------------------------------------------------------
    def _wopbs(self, ct_in: RadixBatch, lut, nbits: list, delta_log: int) -> RadixBatch:
        p = self.param
        eng = self.wopbs_key.engine
        data, back = self._host(ct_in)
        K, nb = data.shape[0], data.shape[1]
        order = [j for j in range(nb - 1, -1, -1) if nbits[j]]      # most significant block first
        if not order:
            raise ValueError("wopbs: no bit to extract (every block has degree 0)")
        groups = {}
        for j in order:
            groups.setdefault(nbits[j], []).append(j)
        bits_of = {}
        for n, blocks in groups.items():                           # one extract_bits call per bit count
            b = eng.extract_bits(np.concatenate([data[:, j, :] for j in blocks]), delta_log, n)
            for q, j in enumerate(blocks):
                bits_of[j] = b[q * K:(q + 1) * K]
        bits = np.concatenate([bits_of[j] for j in order], axis=1)  # [K][total_bits][n+1]
        lut = np.ascontiguousarray(lut, dtype=np.uint64)
        if lut.ndim != 2 or lut.shape[1] != self._lut_size(bits.shape[1]):
            raise ValueError(f"wopbs: the LUT must be [outputs][{self._lut_size(bits.shape[1])}] for "
                             f"{bits.shape[1]} extracted bits")
        out = self.wopbs_key.circuit_bootstrapping_vertical_packing(lut, bits)
        keep = min(nb, lut.shape[0])                                # zip(blocks, outputs)
        return RadixBatch(back(np.ascontiguousarray(out[:, :keep])), [p.message_modulus - 1] * keep,
                          [NOISE_NOMINAL] * keep)

    def wopbs(self, ct_in: RadixBatch, lut) -> RadixBatch:
        """integer/wopbs/mod.rs:277-341: one bit of padding, ceil(log2(degree + 1)) bits per block."""
        p = self.param
        delta_log = ((1 << 63) // (p.message_modulus * p.carry_modulus)).bit_length() - 1
        return self._wopbs(ct_in, lut, [_ceil_log2(d + 1) for d in ct_in.degree], delta_log)

    def wopbs_without_padding(self, ct_in: RadixBatch, lut) -> RadixBatch:
        """integer/wopbs/mod.rs:365-428: no padding bit, log2(message carry) bits per block."""
        p = self.param
        block_modulus = p.message_modulus * p.carry_modulus
        delta_log = ((1 << 63) // (block_modulus // 2)).bit_length() - 1
        return self._wopbs(ct_in, lut, [int(np.log2(block_modulus))] * ct_in.num_blocks, delta_log)

    def bivariate_wopbs_with_degree(self, ct1: RadixBatch, ct2: RadixBatch, lut) -> RadixBatch:
        """integer/wopbs/mod.rs:487-493: wopbs of ct1's blocks followed by ct2's; the LUT's outputs pair with
        the first blocks, ct1's."""
        d1, _ = self._host(ct1)
        d2, _ = self._host(ct2)
        _, back = self._host(ct1)
        both = RadixBatch(np.concatenate([d1, d2], axis=1), list(ct1.degree) + list(ct2.degree),
                          list(ct1.noise) + list(ct2.noise))
        res = self.wopbs(both, lut)
        return RadixBatch(back(res.data), res.degree, res.noise)

    # -- between the PBS and the WoP parameter sets --------------------------------------------
    def keyswitch_to_wopbs_params(self, sks, ct_in: RadixBatch) -> RadixBatch:
        """shortint keyswitch_to_wopbs_params (wopbs/mod.rs:724-754) on every block: ONE identity KS+PBS
        launch under the PBS set over the non-trivial blocks, ONE keyswitch PBS big key -> WoP big key over
        all of them.  Degrees are kept."""
        wk = self.wopbs_key
        if wk.ksk_pbs_to_wopbs is None:
            raise ValueError("keyswitch_to_wopbs_params: a key only for wopbs has no PBS -> WoP keyswitching key")
        s = self._shortint(sks)
        data, back = self._host(ct_in)
        K, nb, w = data.shape
        clean = data.copy()
        live = [j for j in range(nb) if ct_in.noise[j] != NOISE_ZERO]
        if live:
            acc = s.generate_lookup_table(lambda x: x)
            rows = np.ascontiguousarray(data[:, live, :]).reshape(-1, w)
            clean[:, live, :] = s.engine_ks_pbs(rows, acc.acc).reshape(K, len(live), w)
        out = wk.engine.keyswitch_with_key(wk.ksk_pbs_to_wopbs, clean.reshape(K * nb, w))
        return RadixBatch(back(out.reshape(K, nb, -1)), list(ct_in.degree), [NOISE_NOMINAL] * nb)

    def keyswitch_to_pbs_params(self, ct_in: RadixBatch) -> RadixBatch:
        """shortint keyswitch_to_pbs_params (wopbs/mod.rs:660-722) on every block: ONE keyswitch WoP big key
        -> PBS small key, ONE identity PBS under the PBS set."""
        wk = self.wopbs_key
        ps = wk.pbs_server_key
        data, back = self._host(ct_in)
        K, nb, w = data.shape
        rows = data.reshape(K * nb, w)
        small = ps.engine.keyswitch(rows) if wk.ksk_wopbs_to_pbs is None else \
            ps.engine.keyswitch_with_key(wk.ksk_wopbs_to_pbs, rows)
        out = ps.engine.programmable_bootstrap(small, ps.generate_lookup_table(lambda x: x).acc)
        return RadixBatch(back(out.reshape(K, nb, -1)), list(ct_in.degree), [NOISE_NOMINAL] * nb)


class ClientKey:
    """integer RadixClientKey over a shortint ClientKey (integer/client_key/radix.rs)."""

    def __init__(self, shortint_client_key, num_blocks: int):
        self.key = shortint_client_key
        self.num_blocks = num_blocks

    def encrypt(self, values) -> RadixBatch:
        """Radix decomposition, least significant block first (integer/client_key/mod.rs)."""
        p = self.key.parameters
        v = np.asarray(values, dtype=np.uint64)
        m = np.uint64(p.message_modulus)
        bits = int(np.log2(p.message_modulus))
        digits = [(v >> np.uint64(bits * j)) % m for j in range(self.num_blocks)]
        blocks = [self.key.encrypt_many(d) for d in digits]   # each: list of K shortint cts
        data = np.stack([np.stack([c.ct for c in blk]) for blk in blocks], axis=1)
        return RadixBatch(data, [p.message_modulus - 1] * self.num_blocks, [NOISE_NOMINAL] * self.num_blocks)

    def decrypt(self, rb: RadixBatch) -> np.ndarray:
        p = self.key.parameters
        from . import client

        if not isinstance(rb.data, np.ndarray):
            rb = RadixBatch(rb.data.cpu().numpy().view(np.uint64), rb.degree, rb.noise)
        bits = int(np.log2(p.message_modulus))
        out = np.zeros(rb.count, dtype=np.uint64)
        for j in range(rb.num_blocks):
            raw = client.lwe_decrypt(self.key.large_lwe_secret_key, np.ascontiguousarray(rb.data[:, j, :]))
            d = client.decode(raw, p.delta) % np.uint64(p.message_modulus)
            out += d << np.uint64(bits * j)
        return out

    def encrypt_without_padding(self, values) -> RadixBatch:
        """The radix digits under the encoding without a padding bit (shortint encrypt_without_padding)."""
        p = self.key.parameters
        v = np.asarray(values, dtype=np.uint64)
        bits = int(np.log2(p.message_modulus))
        digits = [(v >> np.uint64(bits * j)) % np.uint64(p.message_modulus) for j in range(self.num_blocks)]
        blocks = [self.key.encrypt_without_padding_many(d) for d in digits]
        data = np.stack([np.stack([c.ct for c in blk]) for blk in blocks], axis=1)
        return RadixBatch(data, [p.message_modulus - 1] * self.num_blocks, [NOISE_NOMINAL] * self.num_blocks)

    def decrypt_without_padding(self, rb: RadixBatch) -> np.ndarray:
        p = self.key.parameters
        from . import client

        if not isinstance(rb.data, np.ndarray):
            rb = RadixBatch(rb.data.cpu().numpy().view(np.uint64), rb.degree, rb.noise)
        bits = int(np.log2(p.message_modulus))
        out = np.zeros(rb.count, dtype=np.uint64)
        for j in range(rb.num_blocks):
            raw = client.lwe_decrypt(self.key.large_lwe_secret_key, np.ascontiguousarray(rb.data[:, j, :]))
            d = client.decode(raw, 2 * p.delta) % np.uint64(p.message_modulus)
            out += d << np.uint64(bits * j)
        return out
