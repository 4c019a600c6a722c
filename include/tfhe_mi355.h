/*
 * tfhe_mi355.h -- C ABI of the MI355X programmable-bootstrap engine.
 *
 * This is the drop-in boundary for the reference's PBS hot path (tfhe-rs-odd = tfhe 0.5.0
 * fork, CPU-only Rust).  Each entry point names the reference interface it replaces.  The
 * Rust-side binding a maintainer would add (a `ShortintBootstrappingKey::Gpu` arm calling
 * these functions through `extern "C"`) is shown in INTEGRATION.md.
 *
 * Conventions (mirroring tfhe/src/c_api/utils.rs:3-73 and c_api/core_crypto/mod.rs:37-121):
 *   - every function returns int: 0 = success, 1 = failure; the failure text is returned by
 *     tfhe_mi355_last_error() (thread-local);
 *   - out-params of handle type are nulled first (c_api/shortint/server_key/pbs.rs:25-28);
 *   - buffers are plain uint64_t arrays in the reference's entity layouts:
 *       LWE ciphertext   = mask[0..n) || body                      (lwe_ciphertext.rs:598-599)
 *       GLWE ciphertext  = k mask polys || body poly, N coeffs each (glwe_ciphertext.rs:423-425)
 *       standard BSK     = [n][L][k+1 rows][k+1 polys][N]          (ggsw_ciphertext.rs:185-216)
 *       multi-bit BSK    = [n/g][2^g][L][k+1][k+1][N]              (lwe_multi_bit_bootstrap_key.rs)
 *       KSK              = [in_dim][L_ks][out_dim+1], levels stored L..1
 *                          (lwe_keyswitch_key.rs:102-108, lwe_keyswitch_key_generation.rs:109)
 *       relin. key       = [k(k+1)/2][L][k+1 polys][N], level L first
 *                          (custom_glwe_relinearization_key.rs, custom_relinearization_key_generation.rs:134-138);
 *   - "_async" entry points take DEVICE pointers and a hipStream_t (as void*), enqueue the work
 *     and return immediately; the others take HOST pointers and return after the outputs are
 *     written (synchronous).  The host-pointer forms pipeline the batch in chunks through
 *     page-locked staging on two streams (copies of one chunk overlap the kernels of the next);
 *   - a context is bound to one GPU (tfhe_mi355_context_create) or to a list of GPUs
 *     (tfhe_mi355_context_create_devices: keys replicated, batches split over the devices, see
 *     there); host-pointer calls on one context are thread-safe, so
 *     rayon-style concurrent callers sharing a key are safe (SURVEY.md 8b "Threading"): calls of
 *     more than 64 ciphertexts are serialised by an internal mutex, smaller concurrent calls of
 *     the same entry point are coalesced into shared batches that a dispatcher thread of the
 *     context runs on its own stream, each caller blocking until its own rows are written
 *     (a batch closes when no call has arrived for TFHE_MI355_COALESCE_GAP_US = 50, after at most
 *     _WINDOW_US = 1000, at _BATCH = 1024 ciphertexts, or -- blocking callers only -- as soon as
 *     as many rows are queued as the previous batch of the entry point had; _SLOTS, _OVERFLOW: a
 *     second batch runs concurrently only when half a batch is queued; a call that finds the
 *     coalescer idle runs at once on the calling thread, TFHE_MI355_COALESCE_DIRECT=0 turns that
 *     off; the one-ciphertext-per-call pattern, shortint/server_key/mod.rs:783-857;
 *     TFHE_MI355_COALESCE_MAX_COUNT=0 turns coalescing off).  At N = 2048, k = 1, L = 1, batches
 *     of at most three (classic) / two (multi-bit g = 2, 3) passes of one ciphertext per CU (768 /
 *     512 rows on 256 CUs: the measured crossovers against the throughput kernels) run the
 *     one-ciphertext-per-CU latency kernels (same outputs; TFHE_MI355_LATENCY_MAX = rows
 *     overrides, 0 = never).  At N = 8192 / 4096, k = 1, L = 1 or 2 (classic), batches of at least
 *     3/8 / 5/8 of the CU count (96 / 160 rows on 256 CUs) run the on-chip CMUX (the whole blind
 *     rotation in one workgroup per ciphertext, two per CU at N = 4096, no scratch used), smaller
 *     ones the split CMUX (same outputs; TFHE_MI355_ONCHIP_MIN = rows overrides,
 *     TFHE_MI355_ONCHIP=0 = never); at N = 8192 / 4096 (L = 1 or 2) batches of at most CUs / 4 / CUs / 2
 *     rows run the quad CMUX instead (four / two CUs per ciphertext exchanging sub-blocks every CMUX
 *     through the scratch; same outputs; TFHE_MI355_QUAD_MAX = rows overrides, TFHE_MI355_QUAD=0 =
 *     never).  The quad
 *     CMUX's workgroups wait on each other, so its launches are serialised per device within the
 *     process; two PROCESSES running quad CMUX kernels on one GPU at once can starve each other's
 *     workgroups -- the waits are bounded, and a synchronous call whose quad launch timed out
 *     fails (rc 1, outputs invalid) instead of hanging (an _async call's failure is reported by
 *     the context's next synchronous call); set TFHE_MI355_QUAD=0 where processes share a GPU.
 *     The _async calls hold no per-context mutable state: every device scratch buffer they
 *     need comes from the caller (d_scratch, sized by the matching *_scratch query; a call
 *     given less than its query fails with an error, and only a query returning 0 allows
 *     d_scratch = NULL), so concurrent callers on different streams only need scratch buffers
 *     of their own, and the calls can be captured into a hipGraph (no allocation or
 *     synchronisation inside).  Two forms are the exception:
 *     tfhe_mi355_bootstrap_key_convert_async and tfhe_mi355_keyswitch_key_upload_async wait for
 *     their stream before they return (see "keys uploaded through the _async/device forms" below),
 *     so they refuse a capturing stream: rc 1 and a message naming stream capture, before anything
 *     is locked, marked not ready or enqueued -- the caller's capture stays valid and the resident
 *     key is untouched; upload keys outside the graph.  No warm-up is needed: the first call of a
 *     form on a context may be the captured one (an _async call initialises nothing lazily).
 *     The per-device serialisation of quad CMUX launches does not extend to captured graphs: the
 *     launcher skips its cross-stream event chain while the stream is being captured, so a replay
 *     is ordered against nothing.  Do not replay a graph that holds a quad CMUX while another quad
 *     launch, eager or replayed, may run on the same GPU;
 *   - every device pointer handed to an _async entry point (inputs, outputs, LUTs, index and opcode
 *     arrays, Fourier GGSW lists, key sources, d_scratch) must be 16-byte aligned at its base; rows
 *     inside a buffer follow from the row lengths (8-byte alignment for u64 rows, 4 for u32 rows, 16
 *     for u128 rows).  Nothing needs more: the calls are tested with every base at 16 modulo 256.
 *     An _async call writes nothing outside rows [0, count) of its output (for the strided calls:
 *     the words the call names) and bytes [0, scratch_bytes) of d_scratch -- not its inputs, not a
 *     byte next to either -- and its result does not depend on what the output or the scratch held
 *     before the call (in-place operands excepted: they are inputs);
 *   - keys: a key upload (any *_key_upload*, *_set_ready) waits for the coalesced batches in
 *     flight and blocks new ones until it is done (a pending upload also keeps new batches from
 *     starting, so uploads are not starved under load); the serialized-key uploads hold the key
 *     lock from their first key write to the ready flag; a caller that fills the buffer of
 *     tfhe_mi355_bootstrap_key_fourier / _keyswitch_key_device itself owns that window (calls made
 *     before its _set_ready see whatever the buffer holds; on a multi-device context the hand-out
 *     marks that key not uploaded on every device, so batched calls fail until _set_ready, which
 *     replicates the buffer to the other devices); _async calls are not ordered with
 *     uploads: do not re-upload a key while _async work that reads it may still run;
 *   - _async lut index arrays are not checked on the host (they live on the device): an entry
 *     >= lut_count is clamped to lut_count - 1 by the kernels (no out-of-bounds read); the
 *     host-pointer forms reject such an entry with an error;
 *   - keys uploaded through the _async/device forms are complete when the upload call returns
 *     (it waits for its stream), so any later call on any stream sees the whole key.
 */
#ifndef TFHE_MI355_H
#define TFHE_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHE_MI355_OK 0
#define TFHE_MI355_ERROR 1

typedef struct TfheMi355Context TfheMi355Context;

/* Parameter set.  Mirrors shortint ClassicPBSParameters / MultiBitPBSParameters
 * (shortint/parameters/mod.rs:60-75, multi_bit.rs:173-190). grouping_factor = 0: classic PBS. */
typedef struct {
    uint32_t lwe_dimension;   /* n: small LWE dimension (PBS input)            */
    uint32_t glwe_dimension;  /* k                                             */
    uint32_t polynomial_size; /* N                                             */
    uint32_t pbs_base_log;
    uint32_t pbs_level;
    uint32_t ks_base_log;
    uint32_t ks_level;
    uint32_t message_modulus;
    uint32_t carry_modulus;
    uint32_t grouping_factor; /* 0 = classic; 2, 3 = multi-bit: N = 2048 (k = 1, L = 1),
                                 N = 512 (k = 3, L = 1), N = 8192 (k = 1, L = 2)  */
} TfheMi355Parameters;

/* Thread-local text of the last failure ("" if none). */
const char *tfhe_mi355_last_error(void);

/* Number of visible GPUs. */
int tfhe_mi355_device_count(int *out_count);

/* Per-kernel timing (profiling aid; the counterpart of the reference's `__profiling` feature,
 * tfhe/Cargo.toml:131, which un-inlines the FFT and external-product pieces for perf): with
 * `every` > 0 the device launchers of this context bracket every `every`-th launch of each kernel
 * family with HIP events on the launch stream (never while the stream is being captured);
 * `every` = 0 turns it off.  Enabling clears earlier totals.  Entries are read one by one:
 * index -> (kernel family name, total ms, timed launches); the call waits for the recorded
 * events and fails past the last entry. */
int tfhe_mi355_kernel_timing_enable(TfheMi355Context *ctx, int every);
int tfhe_mi355_kernel_timing_entry(TfheMi355Context *ctx, size_t index, char *name, size_t name_len,
                                   double *total_ms, uint64_t *launches);

/* Asynchronous form of the small host-pointer calls (the coalescer's queue):
 * tfhe_mi355_submit enqueues 1..1024 ciphertexts of one op (0: programmable_bootstrap,
 * 1: keyswitch_programmable_bootstrap, 2: programmable_bootstrap_keyswitch, 3: keyswitch; arguments
 * as those entry points, luts ignored for op 3) and returns at once with a request handle;
 * tfhe_mi355_wait blocks until the outputs are written and frees the handle (every submitted
 * request must be waited on exactly once, before the buffers are reused or the context is
 * destroyed; a request still queued when tfhe_mi355_context_destroy runs is not run: destroy
 * returns 1, and that request's wait returns 1 with a message).  One thread can keep many requests in flight: a rayon worker can submit every block
 * of its share of an integer layer, then wait for them (the reference calls
 * keyswitch_programmable_bootstrap_assign per block, shortint/server_key/mod.rs:783-857), so the
 * coalesced batch is no longer capped by the number of threads. */
typedef struct TfheMi355Request TfheMi355Request;
int tfhe_mi355_submit(TfheMi355Context *ctx, int op, const uint64_t *lwe_in, uint64_t *lwe_out,
                      const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count,
                      TfheMi355Request **out_req);
int tfhe_mi355_wait(TfheMi355Request *req);

/* Request-coalescing counters of this context (all ops): batches run, ciphertexts in them, the
 * most batches in flight at once, and the summed wall time of the batches (staging, copies,
 * kernels, sync); `reset` != 0 clears them after reading.  Profiling aid, no reference
 * counterpart (the reference has no batching layer). */
int tfhe_mi355_coalesce_stats(TfheMi355Context *ctx, int reset, uint64_t *batches, uint64_t *rows,
                              uint64_t *max_in_flight, double *batch_seconds);

/* Page-locked (pinned) host memory for batch buffers.  The synchronous host-pointer entry points
 * detect pinned input/output buffers and DMA them directly, chunk by chunk, overlapped with the
 * kernels (no host staging copies); pageable buffers go through the engine's pinned staging.
 * A Rust binding allocates its LWE batch Vecs here to get the device rate over PCIe.
 * (No reference counterpart: the reference is CPU-only; the buffers replace Vec<u64> batches.) */
int tfhe_mi355_host_alloc(size_t bytes, void **out_ptr);
int tfhe_mi355_host_free(void *ptr);

/* Create / destroy an engine context on `device`.
 * Accepted decompositions: 2 <= pbs_base_log and pbs_base_log * pbs_level <= 30 for N <= 2048 and
 * multi-bit; <= 63 for classic N >= 4096, with pbs_base_log <= 15 when pbs_level > 1 (the split
 * CMUX packs signed digits into int16) and pbs_base_log <= 31 when pbs_level = 1 (it computes them
 * as int32).  Every reference parameter set is inside these bounds.
 * Replaces Fft::new + the shortint engine's thread-local buffers
 * (fft64/math/fft/mod.rs:146-193, shortint/engine/mod.rs:23-70,163-235). */
int tfhe_mi355_context_create(const TfheMi355Parameters *params, int device,
                              TfheMi355Context **out_ctx);
/* One context over several GPUs of this process (SURVEY.md 8b ctx_create(params, device_mask);
 * the reference's one process with its rayon pool, shortint/engine/mod.rs:23-25, calling one KS+PBS
 * per block from par_iter, integer/server_key/radix_parallel/mul.rs:347-407).  `devices` lists
 * device ordinals (a device may repeat: its shards then run side by side on their own streams);
 * devices = NULL with device_count = 0 takes every visible device; one device is the same as
 * tfhe_mi355_context_create.  Behaviour of every entry point on such a context:
 *   - key uploads (host or device pointer, seeded, serialized, the _fourier/_device + _set_ready
 *     pairs) go to the first device and are replicated from its memory: RCCL ncclBroadcast among
 *     the distinct devices (one rank per device, over xGMI; librccl is opened at run time), then
 *     device-to-device copies to further shards of the same device (TFHE_MI355_REPLICATE=copy:
 *     peer copies instead of RCCL; the default "auto" also falls back to peer copies when librccl
 *     cannot be loaded or its communicator is refused); device-pointer key inputs live on the first
 *     device.  Peer access is enabled between the distinct devices at creation.  A failed upload
 *     or replication leaves that key part not uploaded on EVERY device;
 *   - the calling thread's current HIP device is left as it was by every entry point;
 *   - batched host-pointer calls (PBS, KS, KS->PBS, PBS->KS, blind rotation, packing KS,
 *     GLWE products) are split into contiguous row shares, one per device, run concurrently and
 *     joined before the call returns; outputs are bit-identical to a single-device context;
 *   - calls of at most TFHE_MI355_COALESCE_MAX_COUNT ciphertexts and tfhe_mi355_submit go to the
 *     devices' coalescers in turn (round robin);
 *   - device-pointer (_async) calls and the *_scratch queries address the FIRST device (a device
 *     pointer belongs to one GPU): use tfhe_mi355_context_device_context for the others;
 *   - kernel timing and coalescing statistics are summed over the devices. */
int tfhe_mi355_context_create_devices(const TfheMi355Parameters *params, const int *devices, size_t device_count,
                                      TfheMi355Context **out_ctx);
/* How the last key replication of a context ran: TFHE_MI355_REPLICATION_NONE (a single-device
 * context, or nothing replicated yet), _RCCL (ncclBroadcast), _PEER_COPY (hipMemcpyPeerAsync between
 * distinct devices), _DEVICE_COPY (one distinct device: device-to-device copies only).  `note`
 * (optional, borrowed until the next upload) says why auto mode did not use RCCL, else "". */
#define TFHE_MI355_REPLICATION_NONE 0
#define TFHE_MI355_REPLICATION_RCCL 1
#define TFHE_MI355_REPLICATION_PEER_COPY 2
#define TFHE_MI355_REPLICATION_DEVICE_COPY 3
int tfhe_mi355_context_replication(TfheMi355Context *ctx, int *mode, const char **note);
/* Number of devices (shards) of a context: 1 for a single-device context. */
int tfhe_mi355_context_devices(TfheMi355Context *ctx, size_t *count);
/* The single-device context of shard `index` and its device ordinal (borrowed: owned and destroyed
 * by `ctx`; destroying it directly fails).  For a single-device context, index 0 is ctx itself. */
int tfhe_mi355_context_device_context(TfheMi355Context *ctx, size_t index, TfheMi355Context **out_ctx,
                                      int *device);
/* Destroy stops the request coalescer first (a batch already running completes), then frees the
 * device state.  Requests still queued are failed, not run: their tfhe_mi355_wait returns 1, and
 * destroy itself returns 1 saying how many there were (the context is destroyed all the same). */
int tfhe_mi355_context_destroy(TfheMi355Context *ctx);

/* Upload a standard-domain (u64) bootstrapping key and convert it to the engine's Fourier
 * layout on the GPU.  Replaces convert_standard_lwe_bootstrap_key_to_fourier /
 * par_convert_standard_lwe_bootstrap_key_to_fourier (lwe_bootstrap_key_conversion.rs:21-151)
 * and, for grouping_factor > 0, par_convert_standard_lwe_multi_bit_bootstrap_key_to_fourier
 * (lwe_multi_bit_bootstrap_key_conversion.rs).  `len` is in u64 words. */
int tfhe_mi355_bootstrap_key_upload(TfheMi355Context *ctx, const uint64_t *standard_bsk, size_t len);

/* Device-pointer form of the above (standard BSK already in this context's GPU memory). */
int tfhe_mi355_bootstrap_key_convert_async(TfheMi355Context *ctx, const uint64_t *d_standard_bsk,
                                           size_t len, void *stream);

/* Fourier BSK held by the context: device pointer and byte size, for RCCL broadcast of the
 * converted key to the other GPUs of the node. */
int tfhe_mi355_bootstrap_key_fourier(TfheMi355Context *ctx, void **d_ptr, size_t *bytes);
/* (On a context that holds 32-bit-torus keys this returns the Fourier form of the u32 key, same layout,
 * for reading; _set_ready is a 64-bit call and refused there.) */
/* Mark the Fourier BSK as valid after it was filled externally (e.g. by a broadcast into the
 * buffer returned above). */
int tfhe_mi355_bootstrap_key_fourier_set_ready(TfheMi355Context *ctx);

/* Upload a keyswitching key (big LWE key -> small LWE key).  `len` in u64 words. */
int tfhe_mi355_keyswitch_key_upload(TfheMi355Context *ctx, const uint64_t *ksk, size_t len);
/* Device-pointer form of the KSK upload (device-to-device copy on `stream`). */
int tfhe_mi355_keyswitch_key_upload_async(TfheMi355Context *ctx, const uint64_t *d_ksk, size_t len,
                                          void *stream);
int tfhe_mi355_keyswitch_key_device(TfheMi355Context *ctx, void **d_ptr, size_t *bytes);
int tfhe_mi355_keyswitch_key_set_ready(TfheMi355Context *ctx);

/* Batched programmable bootstrap: for c < count,
 *   lwe_out[c] = PBS(lwe_in[c], luts[lut_indexes ? lut_indexes[c] : 0]).
 * lwe_in: count x (n+1); lwe_out: count x (k*N+1); luts: lut_count x (k+1)*N (GLWE accumulators,
 * e.g. from shortint generate_lookup_table).
 * Replaces programmable_bootstrap_lwe_ciphertext[_mem_optimized]
 * (lwe_programmable_bootstrapping.rs:1017-1111) = FourierLweBootstrapKeyView::bootstrap
 * (fft64/crypto/bootstrap.rs:346-380) and, for grouping_factor > 0,
 * multi_bit_programmable_bootstrap_lwe_ciphertext (lwe_multi_bit_programmable_bootstrapping.rs:1035). */
int tfhe_mi355_programmable_bootstrap(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *lwe_out,
                                      const uint64_t *luts, size_t lut_count,
                                      const uint32_t *lut_indexes, size_t count);
int tfhe_mi355_programmable_bootstrap_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in,
                                            uint64_t *d_lwe_out, const uint64_t *d_luts,
                                            size_t lut_count, const uint32_t *d_lut_indexes,
                                            size_t count, void *d_scratch, size_t scratch_bytes,
                                            void *stream);
/* Device scratch (bytes) of the async PBS for `count` ciphertexts (count >= 1):
 *   - classic N <= 2048: 256 bytes (the persistent grid's ciphertext ticket) at the shapes that
 *     run it -- N = 2048 k = 1 L = 1 (every 2_2-like shortint set), N = 1024 k = 1 L = 2,
 *     N = 1024 k = 2 L = 3, N = 256 k = 5 L = 1 -- and 0 at the other classic shapes;
 *   - multi-bit N = 2048 / 512: 0;
 *   - N >= 4096, classic and multi-bit (N = 8192): the accumulators + spectra of one pass of
 *     the split CMUX (also asked for where the on-chip CMUX will run: the call picks by count)
 *     min(count, chunk) ciphertexts (chunk = 128 at N = 32768, 1024 for multi-bit (N = 8192,
 *     400 MiB); otherwise ~200 MiB worth in multiples of 64, at most 1024: 1024 at N = 4096, 512
 *     at N = 8192 (3_3), 256 / 192 at N = 16384, L = 2 / 3; TFHE_MI355_LARGE_CHUNK overrides;
 *     e.g. 1.5 MiB per ciphertext at 4_4).  Less scratch runs smaller passes; the call fails below
 *     one ciphertext's worth.
 * tfhe_mi355_programmable_bootstrap_async fails when given less than this (N <= 2048) -- it never
 * falls back silently.  tfhe_mi355_blind_rotate_async takes no scratch and runs the one-pass grid. */
int tfhe_mi355_programmable_bootstrap_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);

/* Batched blind rotation WITHOUT sample extraction: glwe_out[c] = the rotated accumulator
 * ((k+1)*N words, GLWE layout) of lwe_in[c] with LUT luts[lut_indexes ? lut_indexes[c] : 0].
 * Replaces the fork's FourierLweBootstrapKeyView::bootstrap_without_sample_extract
 * (fft64/crypto/bootstrap.rs:383-412), the first step of its multi-value bootstrapping.
 * Classic and multi-bit contexts with N <= 2048. */
int tfhe_mi355_blind_rotate(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out,
                            const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count);
int tfhe_mi355_blind_rotate_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint64_t *d_glwe_out,
                                  const uint64_t *d_luts, size_t lut_count, const uint32_t *d_lut_indexes,
                                  size_t count, void *stream);

/* The parameter set a context was created with. */
int tfhe_mi355_context_parameters(TfheMi355Context *ctx, TfheMi355Parameters *out);

/* ---- serialized server keys (wire formats; csrc/serde.cpp) ----
 * A tfhe-rs server key arrives as the bincode 1.3.3 encoding of its serde derive
 * (`bincode::serialize(&key)`, tfhe/Cargo.toml:36,57): these entry points take those bytes.
 *   CompressedServerKey (shortint/server_key/compressed.rs:43-55): seeded LWE keyswitching key +
 *     ShortintCompressedBootstrappingKey (Classic / MultiBit seeded BSK) -> regenerated on the GPU
 *     (tfhe_mi355_{keyswitch,bootstrap}_key_upload_seeded).  Replaces
 *     CompressedServerKey::decompress (compressed.rs) + the Fourier conversion.
 *   ServerKey (shortint/server_key/mod.rs:283-297): standard LWE keyswitching key +
 *     Fourier bootstrapping key in concrete-fft's serialized form (FourierPolynomialList,
 *     fft64/math/fft/mod.rs:588-717: natural DFT order), mapped into the engine layout
 *     (every N = 256 ... 32768).  Replaces the ServerKey deserialisation feeding the CPU PBS.
 * Only native (2^64) ciphertext moduli.  *_inspect parses and validates without a GPU and
 * reports the parameter set the key implies (create the context from info.params); *_upload
 * requires a context with exactly that parameter set.  Truncated or inconsistent input fails
 * with a message naming the field and byte offset. */
typedef struct {
    TfheMi355Parameters params;        /* implied by the key material (std devs are not serialized) */
    uint32_t pbs_order;                /* PBSOrder: 0 KeyswitchBootstrap, 1 BootstrapKeyswitch */
    uint32_t deterministic_execution;  /* multi-bit keys */
    uint64_t max_degree;
    uint64_t max_noise_level;          /* ServerKey only (a CompressedServerKey has none: 0) */
    uint64_t ksk_seed_lo, ksk_seed_hi; /* CompressedServerKey: CompressionSeed of each key */
    uint64_t bsk_seed_lo, bsk_seed_hi;
} TfheMi355ServerKeyInfo;
int tfhe_mi355_compressed_server_key_inspect(const uint8_t *bytes, size_t len, TfheMi355ServerKeyInfo *info);
int tfhe_mi355_compressed_server_key_upload(TfheMi355Context *ctx, const uint8_t *bytes, size_t len);
int tfhe_mi355_server_key_inspect(const uint8_t *bytes, size_t len, TfheMi355ServerKeyInfo *info);
int tfhe_mi355_server_key_upload(TfheMi355Context *ctx, const uint8_t *bytes, size_t len);
/* engine Fourier layout: freq[e] = natural DFT index held by element e of a polynomial, M = N/2
 * entries, for every N = 256 ... 32768 -- host-only, no GPU needed */
int tfhe_mi355_fourier_engine_frequency(uint32_t N, uint32_t *freq);

/* Seeded (compressed) keys: the reference's SeededLweBootstrapKey / SeededLweKeyswitchKey
 * (shortint CompressedServerKey) hold only the bodies and a CompressionSeed (u128 = hi:lo); every
 * mask is regenerated on the GPU from the concrete-csprng AES-CTR stream of that seed.
 * Replace decompress_seeded_lwe_bootstrap_key (seeded_lwe_bootstrap_key_decompression.rs) +
 * the Fourier conversion, and decompress_seeded_lwe_keyswitch_key
 * (seeded_lwe_keyswitch_key_decompression.rs).  bodies: BSK [ggsw_count][L][k+1][N] (multi-bit:
 * ggsw_count = (n/g) 2^g, grouped as the standard key), KSK [k*N][ks_level]. */
int tfhe_mi355_bootstrap_key_upload_seeded(TfheMi355Context *ctx, const uint64_t *bodies, size_t len,
                                           uint64_t seed_lo, uint64_t seed_hi);
int tfhe_mi355_keyswitch_key_upload_seeded(TfheMi355Context *ctx, const uint64_t *bodies, size_t len,
                                           uint64_t seed_lo, uint64_t seed_hi);
/* the raw mask stream on the device: word w = little-endian bytes [1 + 8w, 9 + 8w) of the
 * AES-CTR table of the seed (concrete-csprng generators/aes_ctr, started at TableIndex::SECOND) */
int tfhe_mi355_csprng_mask_words(TfheMi355Context *ctx, uint64_t seed_lo, uint64_t seed_hi, uint64_t *out,
                                 size_t words);

/* ---- compressed ciphertext ingress --------------------------------------------------------------
 * A client of the reference uploads ciphertexts in one of two compressed forms; the engine expands them
 * on the GPU, so that only the compressed bytes cross PCIe.
 *   shortint::CompactCiphertextList (shortint/ciphertext/mod.rs:521-594): an LweCompactCiphertextList
 *     (entities/lwe_compact_ciphertext_list.rs) under a CompactPublicKey.  Container: [mask_count][n] masks,
 *     then [count] bodies, mask_count = ceil(count / n).  Replaces CompactCiphertextList::expand
 *     (expand_lwe_compact_ciphertext_list, lwe_compact_ciphertext_list_expansion.rs:12-58): row i takes the
 *     mask of bin i / n multiplied by X^(n - (i % n + 1)) in Z[X]/(X^n + 1), and body i.  n is a power of two.
 *   shortint::CompressedCiphertext (mod.rs:467-513): a SeededLweCiphertext<u64>, one body word and a 128-bit
 *     CompressionSeed.  Replaces CompressedCiphertext::decompress (decompress_seeded_lwe_ciphertext,
 *     seeded_lwe_ciphertext_decompression.rs:50-73) for a batch: row r's mask is words [0, n) of the AES-CTR
 *     mask stream of ITS seed (see tfhe_mi355_csprng_mask_words); the key schedule runs on the device.
 *   SeededLweCiphertextList (decompress_seeded_lwe_ciphertext_list, seeded_lwe_ciphertext_list_decompression.rs:
 *     13-100): one seed for the list, row r's mask is words [r n, (r + 1) n) of its stream.
 * Native 2^64 modulus only.  One descriptor names the source; the pointers inside are host pointers for the
 * host-pointer calls and device pointers (16-byte aligned) for the _async calls, the descriptor itself is
 * always host memory and is read before the call returns. */
#define TFHE_MI355_LWE_SOURCE_ROWS 0         /* expanded rows */
#define TFHE_MI355_LWE_SOURCE_COMPACT 1      /* compact list */
#define TFHE_MI355_LWE_SOURCE_SEEDED_LIST 2  /* seeded list, one seed */
#define TFHE_MI355_LWE_SOURCE_SEEDED_ROWS 3  /* seeded ciphertexts, a seed each */
typedef struct {
    uint32_t kind;          /* 0 expanded rows, 1 compact list, 2 seeded list (one seed), 3 seeded rows (a seed each) */
    uint32_t lwe_dimension; /* n of the rows produced (row = n+1 words) */
    const uint64_t *data;   /* 0: [count][n+1]; 1: the compact container; 2, 3: [count] bodies */
    const uint64_t *seeds;  /* 2: {lo, hi}; 3: [count]{lo, hi}; otherwise NULL */
} TfheMi355LweSource;

/* Expansion alone: lwe_out = count rows of n + 1 words.  n is the caller's (it need not be the context's);
 * any context of any width serves, on a multi-device context the first device.  count = 0 is a no-op.
 * Refused (rc 1): an unknown kind, n = 0, kind 1 with n not a power of two, a missing pointer.  The _async
 * form follows the header's rules (no allocation or synchronisation, scratch from the caller, nothing
 * written outside rows [0, count) and [0, scratch_bytes), result independent of earlier contents); its
 * scratch query is 0 for every kind but 2 (the AES tables of the list's seed). */
int tfhe_mi355_lwe_expand(TfheMi355Context *ctx, const TfheMi355LweSource *src, size_t count, uint64_t *lwe_out);
int tfhe_mi355_lwe_expand_scratch(TfheMi355Context *ctx, uint32_t kind, uint32_t lwe_dimension, size_t count,
                                  size_t *bytes);
int tfhe_mi355_lwe_expand_async(TfheMi355Context *ctx, const TfheMi355LweSource *d_src, size_t count,
                                uint64_t *d_lwe_out, void *d_scratch, size_t scratch_bytes, void *stream);

/* Expansion composed with a keyed operation: op as in tfhe_mi355_submit (0 PBS, 1 KS -> PBS, 2 PBS -> KS,
 * 3 KS); the outputs are, bit for bit, those of tfhe_mi355_lwe_expand followed by the operation's own entry
 * point.  The host-pointer form sends the compressed source over PCIe once -- kind 1 whole, kinds 2 and 3 a
 * slice of bodies (and seeds) per chunk of the host pipeline -- and expands each chunk on the device into the
 * buffer the rows would have been copied to (chunks need not respect compact bins).  Kind 0 is the
 * operation's existing call.  luts, lut_count and lut_indexes are ignored for op 3.
 * Refused (rc 1, with a message): src->lwe_dimension other than the operation's input dimension on this
 * context (n for ops 0 and 2, k N for ops 1 and 3); a multi-device context; a context holding 32-bit or
 * 128-bit keys; a missing key.  These calls are not coalesced.  The _async form takes count * (input
 * dimension + 1) words of its scratch for the expanded rows (tfhe_mi355_apply_from_scratch counts them in). */
int tfhe_mi355_apply_from(TfheMi355Context *ctx, int op, const TfheMi355LweSource *src, uint64_t *lwe_out,
                          const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count);
int tfhe_mi355_apply_from_scratch(TfheMi355Context *ctx, int op, uint32_t kind, size_t count, size_t *bytes);
int tfhe_mi355_apply_from_async(TfheMi355Context *ctx, int op, const TfheMi355LweSource *d_src, uint64_t *d_lwe_out,
                                const uint64_t *d_luts, size_t lut_count, const uint32_t *d_lut_indexes, size_t count,
                                void *d_scratch, size_t scratch_bytes, void *stream);

/* The bincode bytes of the two shortint types, parsed without a GPU (field order: ct_list / ct, degree,
 * message_modulus, carry_modulus, pbs_order, noise_level).  The u64 container stays where it is: a caller
 * points TfheMi355LweSource.data at bytes + data_offset (bincode does not align it: copy the data_words words
 * out if bytes + data_offset is not 8-byte aligned).  Truncated or inconsistent input fails with a message
 * naming the field and byte offset; a non-native ciphertext modulus, or a compact container whose length is not
 * lwe_compact_ciphertext_list_size(n, count) (lwe_compact_ciphertext_list.rs:55-63), is refused. */
typedef struct {
    uint32_t lwe_dimension;
    uint32_t pbs_order;    /* PBSOrder: 0 KeyswitchBootstrap, 1 BootstrapKeyswitch */
    uint64_t count;        /* ciphertexts (1 for a CompressedCiphertext) */
    uint64_t degree;
    uint64_t message_modulus;
    uint64_t carry_modulus;
    uint64_t noise_level;
    uint64_t data_offset;  /* byte offset in `bytes` of the container (compact) or of the body word */
    uint64_t data_words;   /* its length in u64 words */
    uint64_t seed_lo, seed_hi; /* CompressedCiphertext: the CompressionSeed */
} TfheMi355CiphertextInfo;
int tfhe_mi355_compact_ciphertext_list_inspect(const uint8_t *bytes, size_t len, TfheMi355CiphertextInfo *info);
int tfhe_mi355_compressed_ciphertext_inspect(const uint8_t *bytes, size_t len, TfheMi355CiphertextInfo *info);

/* LWE -> GLWE packing keyswitch of the fork's tree bootstrapping (gadget ServerKey
 * lwe_packing_keyswitch_key, gadget/engine/bootstrapping.rs:345-352, used at :713,:744).
 * Key layout [k*N][level][(k+1)*N] (levels stored L..1), input key = the big LWE key.
 * Replaces keyswitch_lwe_ciphertext_into_glwe_ciphertext (lwe_packing_keyswitch.rs:102-186):
 * lwe_in count x (k*N+1) -> glwe_out count x (k+1)*N. */
int tfhe_mi355_packing_keyswitch_key_upload(TfheMi355Context *ctx, const uint64_t *pksk, size_t len,
                                            uint32_t base_log, uint32_t level);
int tfhe_mi355_packing_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out, size_t count);
int tfhe_mi355_packing_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint64_t *d_glwe_out,
                                       size_t count, void *d_scratch, size_t scratch_bytes, void *stream);
/* Device scratch (bytes) of the async packing keyswitch.  The packing key's decomposition (base,
 * level) belongs to the key, not to the parameter set: this query fails until the packing key is
 * uploaded, and its answer then depends only on that decomposition and `count`. */
int tfhe_mi355_packing_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);

/* GLWE x plaintext-polynomial products over (Z/2^64)[X]/(X^N+1):
 *   out[c][i] = sum_{j < glwe_per_item} glwe_in[c][j] * polys[i][j]   (each GLWE polynomial)
 * glwe_in [count][glwe_per_item][(k+1)N], polys [npoly][glwe_per_item][N],
 * out [count][npoly][(k+1)N], or [count][npoly][k*N+1] when extract != 0 (degree-0 sample
 * extraction of each product).  Replaces the fork's MVB products v0 * v_i + extraction
 * (gadget/engine/bootstrapping.rs:567-620, polynomial_karatsuba_wrapping_mul at
 * polynomial_algorithms.rs:683-742) and the window sums of pack_into_new_accumulator (:690-773). */
int tfhe_mi355_glwe_poly_mul(TfheMi355Context *ctx, const uint64_t *glwe_in, size_t glwe_per_item,
                             const uint64_t *polys, size_t npoly, size_t count, int extract, uint64_t *out);
int tfhe_mi355_glwe_poly_mul_async(TfheMi355Context *ctx, const uint64_t *d_glwe_in, size_t glwe_per_item,
                                   const uint64_t *d_polys, size_t npoly, size_t count, int extract,
                                   uint64_t *d_out, void *stream);

/* GLWE x GLWE product with relinearisation, the fork's "even transistor" multiplication (glwe_mult,
 * core_crypto/algorithms/custom_glwe_glwe_product.rs:13-321; lwe_mult, gadget/engine/mod.rs:680-751).
 * Relinearisation key layout [k(k+1)/2][level][(k+1)*N] (entities/custom_glwe_relinearization_key.rs):
 * block n = i(i+1)/2 + j (j <= i) holds `level` GLWE encryptions, level L first, of the polynomial
 * (S_i * S_j) << (64 - base_log*lvl) under the GLWE key (custom_relinearization_key_generation.rs:
 * 72-161); its decomposition belongs to the key, 1 <= base_log <= 31, base_log*level <= 63.  On a
 * multi-device context the key goes to every device.
 * glwe_mult: both GLWEs are shifted right by 32 - log_p/2 (log_p even, <= 64), tensored and
 * relinearised: glwe_lhs, glwe_rhs count x (k+1)*N -> out count x (k+1)*N, or count x (k*N+1) when
 * extract != 0 (the degree-0 sample of the product).  lwe_mult: both LWEs (under the big key) are packed
 * by the packing keyswitch (one launch over the 2*count rows; its key must be uploaded too), multiplied
 * and sample-extracted: count x (k*N+1) each.  N a power of two in [256, 2048], 1 <= k <= 5,
 * (k+1)*N <= 4096; anything else fails, as do an odd log_p, a missing key and an `out` that overlaps
 * an input.  The _scratch queries fail until the key(s) are uploaded. */
int tfhe_mi355_relinearization_key_upload(TfheMi355Context *ctx, const uint64_t *rlk, size_t len, uint32_t base_log,
                                          uint32_t level);
int tfhe_mi355_glwe_mult(TfheMi355Context *ctx, const uint64_t *glwe_lhs, const uint64_t *glwe_rhs, uint32_t log_p,
                         int extract, uint64_t *out, size_t count);
int tfhe_mi355_glwe_mult_async(TfheMi355Context *ctx, const uint64_t *d_glwe_lhs, const uint64_t *d_glwe_rhs,
                               uint32_t log_p, int extract, uint64_t *d_out, size_t count, void *d_scratch,
                               size_t scratch_bytes, void *stream);
int tfhe_mi355_glwe_mult_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);
int tfhe_mi355_lwe_mult(TfheMi355Context *ctx, const uint64_t *lwe_lhs, const uint64_t *lwe_rhs, uint32_t log_p,
                        uint64_t *lwe_out, size_t count);
int tfhe_mi355_lwe_mult_async(TfheMi355Context *ctx, const uint64_t *d_lwe_lhs, const uint64_t *d_lwe_rhs,
                              uint32_t log_p, uint64_t *d_lwe_out, size_t count, void *d_scratch,
                              size_t scratch_bytes, void *stream);
int tfhe_mi355_lwe_mult_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);

/* GGSW x GLWE operations on GGSW ciphertexts that are data, not the context's key: every item of a
 * batch brings its own, and the decomposition (base_log, level; base_log * level <= 32) is an
 * argument of the call -- the circuit-bootstrap decomposition of WoP-PBS, not the PBS one.  N in
 * {256, 512, 1024, 2048}, 1 <= k <= 5 (the context's); anything else fails.
 * A GGSW in the standard domain is laid out as one bootstrap-key element, [level 1..L][row k+1]
 * [(k+1)N] u64 with level l at index l-1.  The host-pointer forms take the list in the standard
 * domain and convert it on the device; the _async forms take the Fourier list (engine layout,
 * tfhe_mi355_ggsw_list_fourier_bytes bytes) that tfhe_mi355_ggsw_list_convert_async produces, the
 * device-side convert_standard_ggsw_ciphertext_to_fourier (ggsw_conversion.rs:18-64).
 * ggsw_indexes [count] picks the GGSW of each item (NULL: item i uses GGSW i; ggsw_count >= count).
 *
 * tfhe_mi355_ggsw_external_product: glwe_inout[i] += ggsw[i] (x) glwe_in[i], both [count][(k+1)N].
 * Replaces add_external_product_assign (algorithms/lwe_programmable_bootstrapping.rs:309-473;
 * fft_impl/fft64/crypto/ggsw.rs:477-598).
 * tfhe_mi355_ggsw_cmux: out[i] = ct0[i] + ggsw[i] (x) (ct1[i] - ct0[i]); out == ct0 is allowed, ct1 is
 * left untouched.  Replaces cmux_assign (lwe_programmable_bootstrapping.rs:552-763;
 * fft_impl/fft64/crypto/ggsw.rs:766-777), whose result lands in ct0. */
int tfhe_mi355_ggsw_external_product(TfheMi355Context *ctx, const uint64_t *ggsw_list, size_t ggsw_count,
                                     uint32_t base_log, uint32_t level, const uint32_t *ggsw_indexes,
                                     const uint64_t *glwe_in, uint64_t *glwe_inout, size_t count);
int tfhe_mi355_ggsw_external_product_async(TfheMi355Context *ctx, const void *d_fourier_ggsw, size_t ggsw_count,
                                           uint32_t base_log, uint32_t level, const uint32_t *d_ggsw_indexes,
                                           const uint64_t *d_glwe_in, uint64_t *d_glwe_inout, size_t count,
                                           void *stream);
int tfhe_mi355_ggsw_cmux(TfheMi355Context *ctx, const uint64_t *ggsw_list, size_t ggsw_count, uint32_t base_log,
                         uint32_t level, const uint32_t *ggsw_indexes, const uint64_t *ct0, const uint64_t *ct1,
                         uint64_t *out, size_t count);
int tfhe_mi355_ggsw_cmux_async(TfheMi355Context *ctx, const void *d_fourier_ggsw, size_t ggsw_count,
                               uint32_t base_log, uint32_t level, const uint32_t *d_ggsw_indexes,
                               const uint64_t *d_ct0, const uint64_t *d_ct1, uint64_t *d_out, size_t count,
                               void *stream);
int tfhe_mi355_ggsw_list_fourier_bytes(TfheMi355Context *ctx, size_t ggsw_count, uint32_t level, size_t *bytes);
int tfhe_mi355_ggsw_list_convert_async(TfheMi355Context *ctx, const uint64_t *d_ggsw_list, size_t ggsw_count,
                                       uint32_t level, void *d_fourier_ggsw, void *stream);

/* Vertical packing, the leveled half of WoP-PBS: evaluates a LUT of npoly * N entries at the index
 * whose bits are GGSW-encrypted, most significant first.  ggsw_list [count][nbits] GGSWs, luts
 * [lut_count][npoly][N] with lut_indexes [count] as the PBS takes them (NULL: LUT 0), lwe_out
 * [count][k*N+1].  The first log2(npoly) GGSWs drive a CMUX tree over the LUT polynomials, the
 * others a blind rotation by monomial degrees 1, 2, 4, ... (last GGSW first), then the degree-0
 * sample is extracted.  Replaces vertical_packing (fft_impl/fft64/crypto/wop_pbs/mod.rs:785-853:
 * cmux_tree_memory_optimized :468-592, blind_rotate_assign :866-892).  Fails when npoly is not a
 * power of two, when log2(npoly) > nbits (the reference then skips the tree and reads one
 * polynomial only), when nbits - log2(npoly) > log2(N), or when nbits = 0.
 * Launches: one per tree level, over count * (npoly >> (level + 1)) CMUX nodes, then one for the whole
 * blind rotation: every item's nbits - log2(npoly) rotation steps and its sample extraction run back
 * to back inside it (timer families ggsw_cmux_tree, ggsw_rotate_chain).  Without rotation bits the last
 * tree level extracts.  TFHE_MI355_VP_STEPWISE=1 launches the rotation steps one by one instead
 * (ggsw_rotate; same results, for A/B runs).  TFHE_MI355_GGSW_GRID=<n>, read at every launch, caps the
 * workgroups of a GGSW launch (a test hook: the persistent node loop then wraps at small counts).
 * The _async form takes the Fourier GGSW list and tfhe_mi355_vertical_packing_scratch bytes of device
 * scratch (the tree's two ping-pong accumulator lists, count * max(npoly/2, 1) and count * max(npoly/4, 1)
 * GLWEs, each rounded up to 256 bytes; the first also holds the rotation's accumulators); a NULL or short
 * scratch fails. */
int tfhe_mi355_vertical_packing(TfheMi355Context *ctx, const uint64_t *ggsw_list, uint32_t base_log, uint32_t level,
                                uint32_t nbits, const uint64_t *luts, size_t lut_count, size_t npoly,
                                const uint32_t *lut_indexes, size_t count, uint64_t *lwe_out);
int tfhe_mi355_vertical_packing_async(TfheMi355Context *ctx, const void *d_fourier_ggsw, uint32_t base_log,
                                      uint32_t level, uint32_t nbits, const uint64_t *d_luts, size_t lut_count,
                                      size_t npoly, const uint32_t *d_lut_indexes, size_t count, uint64_t *d_lwe_out,
                                      void *d_scratch, size_t scratch_bytes, void *stream);
int tfhe_mi355_vertical_packing_scratch(TfheMi355Context *ctx, size_t npoly, size_t count, size_t *bytes);

/* The bootstrapped half of WoP-PBS: LWE ciphertexts in, looked-up LWE ciphertexts out, all on the
 * device (extract_bits -> circuit_bootstrap_boolean -> vertical_packing,
 * fft_impl/fft64/crypto/wop_pbs/mod.rs:66-225, 243-444, 647-746).  It needs a classic PBS shape with
 * N <= 2048 and k <= 5, the context's bootstrapping and keyswitching keys, and the private functional
 * packing keyswitching keys:
 *
 * pfpksk list: the reference's LwePrivateFunctionalPackingKeyswitchKeyList memory as it is,
 * [k+1 keys][k*N+1 input blocks][level][(k+1)*N], level 1 first (the opposite of the keyswitching and
 * packing keys' L..1 order: no flipping by the caller).  Its decomposition belongs to the key:
 * 1 <= base_log <= 31, level >= 1, base_log * level <= 63.  A multi-device context uploads it to every
 * device. */
int tfhe_mi355_pfpksk_list_upload(TfheMi355Context *ctx, const uint64_t *pfpksk, size_t len, uint32_t base_log,
                                  uint32_t level);
/* private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext
 * (lwe_private_functional_packing_keyswitch.rs:21-89) under every key of the list:
 * lwe_in [count][k*N+1] -> glwe_out [count][k+1][(k+1)*N],
 * glwe_out[c][g] = - sum_i sum_lvl digit_lvl(lwe_in[c][i]) * key_g[i][lvl], the body (i = k*N) decomposed
 * like the mask words and not added to the output.  base_log <= 15 runs as int8 MFMA GEMMs on byte
 * planes repacked at upload, wider digits in a 64-bit integer kernel; both are exact.  The scratch
 * query fails until the keys are uploaded. */
int tfhe_mi355_private_functional_packing_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out,
                                                    size_t count);
int tfhe_mi355_private_functional_packing_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in,
                                                          uint64_t *d_glwe_out, size_t count, void *d_scratch,
                                                          size_t scratch_bytes, void *stream);
int tfhe_mi355_private_functional_packing_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);
/* extract_bits (wop_pbs/mod.rs:66-225): lwe_in [count][k*N+1] -> lwe_out [count][nbits][n+1], the bits
 * delta_log .. delta_log + nbits - 1 of every message, most significant first, each scaled to q/2 and
 * under the small LWE key.  Fails when delta_log + nbits > 64, nbits = 0, or delta_log = 0 with
 * nbits > 1 (the reference's shift underflows there). */
int tfhe_mi355_extract_bits(TfheMi355Context *ctx, const uint64_t *lwe_in, uint32_t delta_log, uint32_t nbits,
                            uint64_t *lwe_out, size_t count);
int tfhe_mi355_extract_bits_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint32_t delta_log, uint32_t nbits,
                                  uint64_t *d_lwe_out, size_t count, void *d_scratch, size_t scratch_bytes,
                                  void *stream);
int tfhe_mi355_extract_bits_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);
/* circuit_bootstrap_boolean (wop_pbs/mod.rs:243-444): lwe_in [count][n+1], one bit at 2^delta_log each
 * -> ggsw_out [count][cbs_level][k+1][(k+1)*N], standard domain, the layout
 * tfhe_mi355_ggsw_list_convert_async and the host-pointer GGSW calls take.  One PBS launch over
 * count * cbs_level rows and one pfpks launch over the same rows.  cbs_base_log * cbs_level <= 32. */
int tfhe_mi355_circuit_bootstrap(TfheMi355Context *ctx, const uint64_t *lwe_in, uint32_t delta_log,
                                 uint32_t cbs_base_log, uint32_t cbs_level, uint64_t *ggsw_out, size_t count);
int tfhe_mi355_circuit_bootstrap_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint32_t delta_log,
                                       uint32_t cbs_base_log, uint32_t cbs_level, uint64_t *d_ggsw_out, size_t count,
                                       void *d_scratch, size_t scratch_bytes, void *stream);
int tfhe_mi355_circuit_bootstrap_scratch(TfheMi355Context *ctx, uint32_t cbs_level, size_t count, size_t *bytes);
/* circuit_bootstrap_boolean_vertical_packing (wop_pbs/mod.rs:647-746): lwe_in [count][nbits][n+1], one
 * bit per ciphertext at q/2, most significant first (what tfhe_mi355_extract_bits writes);
 * luts [lut_count][nout][npoly][N] with lut_indexes [count] (NULL: LUT 0); lwe_out [count][nout][k*N+1].
 * Circuit bootstrap, Fourier conversion, then ONE vertical packing over (item, output): output o reads
 * polynomials [o*npoly, (o+1)*npoly) of the item's LUT in place, under the item's GGSWs, so a tree level
 * is one launch over count * nout * (npoly >> (level + 1)) nodes, the rotation one chain launch over
 * count * nout nodes, and the last launch writes lwe_out[item][o] directly (no per-output pass, no LUT
 * gather or output scatter).  Scratch: [standard GGSWs | Fourier GGSWs | max(circuit bootstrap scratch,
 * the vertical packing's ping-pong lists scaled by nout)]; the query returns exactly that. */
int tfhe_mi355_circuit_bootstrap_vertical_packing(TfheMi355Context *ctx, const uint64_t *lwe_in, uint32_t nbits,
                                                  uint32_t cbs_base_log, uint32_t cbs_level, const uint64_t *luts,
                                                  size_t lut_count, size_t nout, size_t npoly,
                                                  const uint32_t *lut_indexes, size_t count, uint64_t *lwe_out);
int tfhe_mi355_circuit_bootstrap_vertical_packing_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint32_t nbits,
                                                        uint32_t cbs_base_log, uint32_t cbs_level,
                                                        const uint64_t *d_luts, size_t lut_count, size_t nout,
                                                        size_t npoly, const uint32_t *d_lut_indexes, size_t count,
                                                        uint64_t *d_lwe_out, void *d_scratch, size_t scratch_bytes,
                                                        void *stream);
int tfhe_mi355_circuit_bootstrap_vertical_packing_scratch(TfheMi355Context *ctx, uint32_t nbits, uint32_t cbs_level,
                                                          size_t lut_count, size_t nout, size_t npoly, size_t count,
                                                          size_t *bytes);

/* Batched LWE keyswitch (big key -> small key): lwe_in count x (k*N+1) -> lwe_out count x (n+1).
 * Replaces keyswitch_lwe_ciphertext (lwe_keyswitch.rs:96-170). */
int tfhe_mi355_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *lwe_out, size_t count);
int tfhe_mi355_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint64_t *d_lwe_out,
                               size_t count, void *d_scratch, size_t scratch_bytes, void *stream);
/* Device scratch (bytes) of the async keyswitch: the int8-MFMA path's digit matrix. */
int tfhe_mi355_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);

/* A keyswitching key as an object of its own, with dimensions no parameter set of the context needs to
 * describe (the keyswitches between a PBS and a WoP-PBS parameter set: big key -> big key of another
 * set, big key -> small key of another set).  ksk is [in_dim][level][out_dim+1], levels L..1: the memory
 * and level order tfhe_mi355_keyswitch_key_upload takes; len must be in_dim * level * (out_dim + 1).
 * Fails on a zero dimension, base_log = 0, level = 0 or base_log * level >= 64.  The key lives on every
 * device of a multi-device context and must be destroyed before the context.
 * tfhe_mi355_keyswitch_with_key: lwe_in count x (in_dim+1) -> lwe_out count x (out_dim+1), the same
 * kernels as tfhe_mi355_keyswitch (int8 MFMA GEMMs where the decomposition allows it, the scalar kernel
 * otherwise; timer family keyswitch); the host form splits the rows over the devices.  The _async form
 * takes tfhe_mi355_keyswitch_with_key_scratch bytes (the MFMA form's digit matrix; 0 for the scalar
 * kernel); a NULL or short scratch fails. */
typedef struct TfheMi355KeyswitchKey TfheMi355KeyswitchKey;
int tfhe_mi355_lwe_keyswitch_key_create(TfheMi355Context *ctx, const uint64_t *ksk, size_t len, size_t in_dim,
                                        size_t out_dim, uint32_t base_log, uint32_t level,
                                        TfheMi355KeyswitchKey **key);
int tfhe_mi355_lwe_keyswitch_key_destroy(TfheMi355KeyswitchKey *key);
int tfhe_mi355_keyswitch_with_key(TfheMi355Context *ctx, const TfheMi355KeyswitchKey *key, const uint64_t *lwe_in,
                                  uint64_t *lwe_out, size_t count);
int tfhe_mi355_keyswitch_with_key_async(TfheMi355Context *ctx, const TfheMi355KeyswitchKey *key,
                                        const uint64_t *d_lwe_in, uint64_t *d_lwe_out, size_t count, void *d_scratch,
                                        size_t scratch_bytes, void *stream);
int tfhe_mi355_keyswitch_with_key_scratch(TfheMi355Context *ctx, const TfheMi355KeyswitchKey *key, size_t count,
                                          size_t *bytes);

/* shortint KS -> PBS (PBSOrder::KeyswitchBootstrap): lwe_in/out count x (k*N+1).
 * Replaces ServerKey::keyswitch_programmable_bootstrap_assign (shortint/server_key/mod.rs:783-857). */
int tfhe_mi355_keyswitch_programmable_bootstrap(TfheMi355Context *ctx, const uint64_t *lwe_in,
                                                uint64_t *lwe_out, const uint64_t *luts, size_t lut_count,
                                                const uint32_t *lut_indexes, size_t count);
int tfhe_mi355_keyswitch_programmable_bootstrap_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in,
                                                      uint64_t *d_lwe_out, const uint64_t *d_luts,
                                                      size_t lut_count, const uint32_t *d_lut_indexes,
                                                      size_t count, void *d_scratch, size_t scratch_bytes,
                                                      void *stream);
/* Device scratch (bytes) needed by the async KS->PBS for `count` ciphertexts: the small-LWE
 * intermediate plus the larger of the keyswitch and PBS scratch. */
int tfhe_mi355_keyswitch_programmable_bootstrap_scratch(TfheMi355Context *ctx, size_t count,
                                                        size_t *bytes);

/* shortint PBS -> KS (PBSOrder::BootstrapKeyswitch): lwe_in/out count x (n+1).
 * Replaces ServerKey::programmable_bootstrap_keyswitch_assign (shortint/server_key/mod.rs:859-932). */
int tfhe_mi355_programmable_bootstrap_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in,
                                                uint64_t *lwe_out, const uint64_t *luts, size_t lut_count,
                                                const uint32_t *lut_indexes, size_t count);
int tfhe_mi355_programmable_bootstrap_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in,
                                                      uint64_t *d_lwe_out, const uint64_t *d_luts,
                                                      size_t lut_count, const uint32_t *d_lut_indexes,
                                                      size_t count, void *d_scratch, size_t scratch_bytes,
                                                      void *stream);
/* Device scratch (bytes) of the async PBS->KS: the big-LWE intermediate plus the larger of the
 * PBS and keyswitch scratch. */
int tfhe_mi355_programmable_bootstrap_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);

/* Batched LWE linear algebra on device rows of u64 words (wrapping mod 2^64):
 *   y[r] = y[r] * scalar + (d_x ? x[r] : 0)   for r < rows, `words` words per row,
 * row strides in words.  Replaces shortint unchecked_add_assign / unchecked_scalar_mul_assign and
 * the bivariate packing left*factor + right (shortint/server_key/bivariate_pbs.rs:167-182) for
 * device-resident radix ciphertexts. */
int tfhe_mi355_lwe_scalar_mul_add_async(TfheMi355Context *ctx, uint64_t *d_y, const uint64_t *d_x, uint64_t scalar,
                                        size_t rows, size_t words, size_t y_stride, size_t x_stride, void *stream);
/* One layer of block arithmetic in one call.  A radix operation alternates batched PBS layers with LWE linear
 * algebra on single blocks: pack two blocks, subtract, negate with a correcting term, add a plaintext to the
 * body (integer/server_key/comparator.rs:182-220, radix/neg.rs:56-73, shortint bivariate_pbs.rs:167-182).  An
 * op describes one destination block as a sum of up to TFHE_MI355_BLOCK_OP_TERMS scaled source blocks; for
 * every op, every row r < rows and every word w < words
 *   dst[r][w] = sum over the present terms of scalar * src[r][w] + (w == words - 1 ? body_add : 0)
 * wrapping mod 2^64, rows `stride` words apart (device pointers, 8-byte aligned).  A term with src == NULL is
 * absent; an op with no term at all writes trivial ciphertexts (zero mask, body = body_add).
 * Aliasing: a term may BE the destination (the same pointer and the same stride: the op then works in place).
 * Any other overlap between a destination and a source or another destination of the same call is the caller's
 * error: the ops of a call run in no defined order, and the result is then undefined.
 * `ops` is host memory and is read before the call returns (the table travels in the kernel arguments, about
 * 32 ops per launch; longer lists take several launches on the stream).  The call needs no scratch, does not
 * allocate, synchronise or copy, and can be captured into a hipGraph, which then holds the table.
 * Refused (rc 1): a NULL dst, a stride below `words`, words == 0 with n_ops > 0.  n_ops == 0 or rows == 0
 * succeeds without a launch. */
#define TFHE_MI355_BLOCK_OP_TERMS 4
typedef struct {
    uint64_t *dst;
    uint64_t dst_stride; /* row r of the block at dst + r * dst_stride (words) */
    uint64_t body_add;   /* added to the last word of every row */
    struct {
        const uint64_t *src;
        uint64_t stride;
        uint64_t scalar;
    } term[TFHE_MI355_BLOCK_OP_TERMS]; /* src == NULL: term absent */
} TfheMi355BlockOp;
int tfhe_mi355_lwe_block_layer_async(TfheMi355Context *ctx, const TfheMi355BlockOp *ops, size_t n_ops,
                                     size_t rows, size_t words, void *stream);
/* The block layer with one clear digit per row.  A clear (unencrypted) operand of a radix operation reaches a
 * PBS layer in one of two ways: as a plaintext on the body of a block (scalar_add / scalar_sub add the scalar's
 * digit times delta, radix/scalar_add.rs:53-65; the order comparisons subtract the packed digit before the sign
 * LUT, comparator.rs:226-238) or as the choice of a LUT out of a small family (x & s, x == s:
 * radix_parallel/scalar_bitwise_op.rs, scalar_comparison.rs:312-336).  This call reads the operand of row r from
 * a device array, so the op table does not depend on it: one table, and one captured graph of it, serves another
 * clear operand in every row and on every replay.  For every op, every row r < rows and every word w < words
 *   c        = d_clear ? (clear_negate ? (0 - d_clear[r]) mod 2^64 : d_clear[r]) : 0
 *   digit(r) = (c >> clear_shift) & (2^clear_bits - 1)        (bits past bit 63 read as 0; clear_bits == 0: 0)
 *   dst[r][w] = sum over the present terms of scalar * src[r][w]
 *               + (w == words - 1 ? body_add + digit(r) * clear_scale : 0)                   wrapping mod 2^64
 *   d_lut_index[r] = lut_base + digit(r)     where d_lut_index != NULL, written exactly once per row.
 * With d_clear == NULL the op is the plain one.  `op`, the aliasing rule, the refusals and the empty calls are
 * those of tfhe_mi355_lwe_block_layer_async; d_clear and d_lut_index overlap no destination.  Also refused
 * (rc 1): clear_shift > 63, clear_bits > 8, d_lut_index != NULL with d_clear == NULL and clear_bits != 0.
 * `ops` is host memory, read before the call returns (about 25 ops per launch travel in the kernel arguments;
 * longer lists take several launches on the stream).  The call needs no scratch, does not allocate, synchronise
 * or copy, and can be captured into a hipGraph. */
typedef struct {
    TfheMi355BlockOp op;
    const uint64_t *d_clear; /* device, one u64 per row; NULL: a plain op */
    uint64_t clear_scale;    /* digit(r) * clear_scale is added to the body of row r */
    uint32_t *d_lut_index;   /* device, one u32 per row, or NULL */
    uint32_t clear_negate;   /* 1: the digit comes from (0 - d_clear[r]) mod 2^64 */
    uint32_t clear_shift;    /* <= 63 */
    uint32_t clear_bits;     /* 0 .. 8 */
    uint32_t lut_base;
} TfheMi355ClearBlockOp;
int tfhe_mi355_lwe_clear_block_layer_async(TfheMi355Context *ctx, const TfheMi355ClearBlockOp *ops, size_t n_ops,
                                           size_t rows, size_t words, void *stream);
/* trivial_pbs_assign (shortint/server_key/mod.rs:763-781) on the bodies of `rows` trivial
 * ciphertexts (d_body points at the first body, rows `stride` words apart) with the GLWE
 * accumulator d_lut ((k+1)*N words, device). */
int tfhe_mi355_trivial_pbs_async(TfheMi355Context *ctx, uint64_t *d_body, size_t rows, size_t stride,
                                 const uint64_t *d_lut, void *stream);

/* Fill a shortint lookup table (GLWE accumulator, (k+1)*N words) from f(i), i < msg*carry.
 * Replaces shortint fill_accumulator (shortint/engine/mod.rs:72-128). */
int tfhe_mi355_fill_accumulator(const TfheMi355Parameters *params, const uint64_t *f_values,
                                uint64_t *accumulator);

/* Diagnostic (test hook, host buffers, synchronous): the PBS kernels' backward torus conversion
 * (x86.rs:823-874 + 961-1044 after the fract) applied to n given fractions fr in [-1/2, 1/2]:
 * acc_inout[i] += X_i and set_out[i] = X_i, X_i = rint_half_even(fr[i] * 2^64) mod 2^64. */
int tfhe_mi355_debug_torus_from_fraction(int device, const double *fr, uint64_t *acc_inout, uint64_t *set_out,
                                         size_t n);
/* Diagnostic: workgroups of the classic u64 PBS kernel of the context's shape resident at once -- the size of
 * its persistent grid, whose slots take further ciphertexts from a ticket (a workgroup holds 4 ciphertexts at
 * N = 2048, k = 1, level 1, otherwise 1); 0 for a shape without a persistent grid.  rc 1 on a context the
 * kernel does not serve (N >= 4096, multi-bit, keys of another torus width).
 * TFHE_MI355_GRID_CAP=<n>, read at every launch, caps that grid, the grid of the AES mask stream of the seeded
 * uploads and expansions, and the row grids of tfhe_mi355_lwe_expand (a test hook: the loops that walk the work
 * beyond the grid then wrap at small counts; unset or 0: no cap; the query above reports the uncapped grid). */
int tfhe_mi355_debug_pbs_resident(TfheMi355Context *ctx, size_t *count);

/* ---- 32-bit torus (the reference's boolean module, tfhe/src/boolean) ----
 * The boolean engine computes on LweCiphertextOwned<u32> under a LweKeyswitchKeyOwned<u32> and the Fourier
 * form of a LweBootstrapKeyOwned<u32> (boolean/engine/bootstrapping.rs:17-97, 158-212).  These entry points
 * run that arithmetic natively: u32 words, the 32-bit signed decomposer, fast_pbs_modulus_switch with
 * Scalar::BITS = 32 and the wrapping f64 -> u32 backward conversion (x86.rs:941-947), the accumulator
 * rounded to 32 bits after every CMUX.  Shapes (N, k, pbs_level): (512, 2, 3), (1024, 2, 2), (1024, 1, 4),
 * (1024, 1, 3) -- the five sets of boolean/parameters/mod.rs:123-192 -- with 2 <= pbs_base_log and
 * pbs_base_log * pbs_level <= 30; any lwe_dimension, ks_base_log * ks_level <= 30.
 *
 * The context is an ordinary tfhe_mi355_context_create one (message_modulus and carry_modulus are not
 * read by these calls).  A context holds keys of ONE torus width: a _u32 upload onto a context that holds
 * u64 keys, a u64 upload onto one that holds u32 keys, and a compute call of the other width than the
 * context's keys all fail with rc 1 and a message.  Not available on a multi-device context (rc 1), not
 * coalesced, no latency kernel: a host-pointer call runs directly under the context's mutex.  The _async
 * forms follow the rules of the u64 ones: device pointers, the caller's stream, no allocation and no
 * synchronisation inside, scratch from the caller (the *_scratch query; too little is an error).
 * count = 0 is a no-op. */

/* Standard u32 bootstrapping key [n][pbs_level][k+1][k+1][N] (host, `len` in u32 words), converted to the
 * Fourier domain on the device: the Fourier key is bit-identical to the conversion of the key widened to
 * u64 (word << 32), since (double)(int32_t)x 2^-32 == (double)(int64_t)((uint64_t)x << 32) 2^-64.
 * Replaces the convert_standard_lwe_bootstrap_key_to_fourier of bootstrapping.rs:173-195. */
int tfhe_mi355_bootstrap_key_upload_u32(TfheMi355Context *ctx, const uint32_t *bsk, size_t len);
/* u32 keyswitching key [kN][ks_level][n+1] (host, `len` in u32 words; bootstrapping.rs:197-206). */
int tfhe_mi355_keyswitch_key_upload_u32(TfheMi355Context *ctx, const uint32_t *ksk, size_t len);

/* programmable_bootstrap_lwe_ciphertext_mem_optimized on u32 (bootstrapping.rs:284-291): lwe_in
 * count x (n+1), lwe_out count x (kN+1), luts lut_count general GLWE accumulators of (k+1)N u32 words,
 * lut_indexes one per ciphertext or NULL (all LUT 0). */
int tfhe_mi355_programmable_bootstrap_u32(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *lwe_out,
                                          const uint32_t *luts, size_t lut_count, const uint32_t *lut_indexes,
                                          size_t count);
int tfhe_mi355_programmable_bootstrap_u32_async(TfheMi355Context *ctx, const uint32_t *d_lwe_in, uint32_t *d_lwe_out,
                                                const uint32_t *d_luts, size_t lut_count,
                                                const uint32_t *d_lut_indexes, size_t count, void *d_scratch,
                                                size_t scratch_bytes, void *stream);
int tfhe_mi355_programmable_bootstrap_u32_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);
/* The same blind rotation without the sample extraction: glwe_out count x (k+1)N. */
int tfhe_mi355_blind_rotate_u32(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *glwe_out,
                                const uint32_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count);
int tfhe_mi355_blind_rotate_u32_async(TfheMi355Context *ctx, const uint32_t *d_lwe_in, uint32_t *d_glwe_out,
                                      const uint32_t *d_luts, size_t lut_count, const uint32_t *d_lut_indexes,
                                      size_t count, void *d_scratch, size_t scratch_bytes, void *stream);
int tfhe_mi355_blind_rotate_u32_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);
/* keyswitch_lwe_ciphertext on u32 (bootstrapping.rs:337-341, 374-378): count x (kN+1) -> count x (n+1). */
int tfhe_mi355_keyswitch_u32(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *lwe_out, size_t count);
int tfhe_mi355_keyswitch_u32_async(TfheMi355Context *ctx, const uint32_t *d_lwe_in, uint32_t *d_lwe_out, size_t count,
                                   void *d_scratch, size_t scratch_bytes, void *stream);
int tfhe_mi355_keyswitch_u32_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);

/* A mixed batch of binary gates (boolean/engine/mod.rs:607-837): item i computes
 * s (lhs[i] + rhs[i]) + (0, ..., 0, c) mod 2^32 with (s, c) of ops[i], T = 1 << 29, F = 7 << 29
 * (boolean/mod.rs:77-80):
 *   0 AND (1, F)   1 NAND (-1, T)   2 NOR (-1, F)   3 OR (1, T)   4 XOR (2, 2T)   5 XNOR (-2, -2T)
 * then apply_bootstrapping_pattern (bootstrapping.rs:392-401) with the constant-T accumulator
 * (bootstrapping.rs:59-60): pbs_order 1 (BootstrapKeyswitch) PBS then keyswitch, rows of n+1 words in and
 * out; pbs_order 0 (KeyswitchBootstrap) keyswitch then PBS, rows of kN+1 words.  ops: count bytes (host
 * for the host-pointer call, which refuses an opcode above 5; device for _async, where such an item
 * bootstraps a row of zeros). */
#define TFHE_MI355_GATE_AND 0
#define TFHE_MI355_GATE_NAND 1
#define TFHE_MI355_GATE_NOR 2
#define TFHE_MI355_GATE_OR 3
#define TFHE_MI355_GATE_XOR 4
#define TFHE_MI355_GATE_XNOR 5
int tfhe_mi355_boolean_gates(TfheMi355Context *ctx, const uint8_t *ops, const uint32_t *lhs, const uint32_t *rhs,
                             uint32_t *out, size_t count, int pbs_order);
int tfhe_mi355_boolean_gates_async(TfheMi355Context *ctx, const uint8_t *d_ops, const uint32_t *d_lhs,
                                   const uint32_t *d_rhs, uint32_t *d_out, size_t count, int pbs_order,
                                   void *d_scratch, size_t scratch_bytes, void *stream);
int tfhe_mi355_boolean_gates_scratch(TfheMi355Context *ctx, size_t count, int pbs_order, size_t *bytes);
/* MUX of encrypted operands (mod.rs:502-566): the rows cond + then + F and -cond + else + F, ONE PBS
 * launch over the 2 count rows, out = pbs1 + pbs2 + T; for pbs_order 1 the keyswitch comes after the
 * sum, for pbs_order 0 before the two bootstraps. */
int tfhe_mi355_boolean_mux(TfheMi355Context *ctx, const uint32_t *cond, const uint32_t *then_ct,
                           const uint32_t *else_ct, uint32_t *out, size_t count, int pbs_order);
int tfhe_mi355_boolean_mux_async(TfheMi355Context *ctx, const uint32_t *d_cond, const uint32_t *d_then,
                                 const uint32_t *d_else, uint32_t *d_out, size_t count, int pbs_order,
                                 void *d_scratch, size_t scratch_bytes, void *stream);
int tfhe_mi355_boolean_mux_scratch(TfheMi355Context *ctx, size_t count, int pbs_order, size_t *bytes);
/* NOT (mod.rs:377-398): d_out[i] = -d_in[i] for `words` u32 words on the device; no key, no PBS. */
int tfhe_mi355_boolean_not_async(TfheMi355Context *ctx, const uint32_t *d_in, uint32_t *d_out, size_t words,
                                 void *stream);

/* Diagnostic (test hook, host buffers, synchronous): the u32 backward conversion's last step
 * (convert_add_backward_torus_u32, x86.rs:877-947) on n fractions fr in [-1/2, 1/2]: acc_inout[i] += X_i
 * and set_out[i] = X_i, X_i = rint_half_even(fr[i] * 2^32) mod 2^32 (fr = +-1/2 give 0x80000000). */
int tfhe_mi355_debug_torus32_from_fraction(int device, const double *fr, uint32_t *acc_inout, uint32_t *set_out,
                                           size_t n);
/* Diagnostic (test hook, host buffers, synchronous): one u32 keyswitch under the caller's key
 * [in_dim][level][out_dim+1] of its own dimensions and decomposition (base_log * level <= 30), through a
 * chosen kernel: arm 0 the engine's choice (the int8-MFMA arm where it takes the shape), 1 the plain
 * integer kernel, 2 the int8-MFMA kernel (rc 1 where that arm does not take the shape).  The key is
 * uploaded, repacked and dropped within the call; the context's keys are not touched. */
int tfhe_mi355_debug_keyswitch_u32(TfheMi355Context *ctx, const uint32_t *ksk, size_t in_dim, size_t out_dim,
                                   uint32_t base_log, uint32_t level, int arm, const uint32_t *lwe_in,
                                   uint32_t *lwe_out, size_t count);
/* Diagnostic: ciphertexts (= workgroups) of the u32 PBS kernel of the context's shape resident at once. */
int tfhe_mi355_debug_pbs_u32_resident(TfheMi355Context *ctx, size_t *count);

/* ---- 128-bit torus (the reference's fft128 path, tfhe/src/core_crypto/fft_impl/fft128) ----
 * programmable_bootstrap_f128_lwe_ciphertext (algorithms/lwe_programmable_bootstrapping.rs:1378-1459) over
 * the Fourier form made by convert_standard_lwe_bootstrap_key_to_fourier_128
 * (algorithms/lwe_bootstrap_key_conversion.rs:164): LweCiphertext<u128>, the 128-bit signed decomposer,
 * fast_pbs_modulus_switch with Scalar::BITS = 128, a negacyclic FFT in double-double arithmetic and the
 * wrapping f128 -> u128 backward conversion (fft128/math/fft/mod.rs:201-328).  The transform's operation
 * order is this engine's own (the reference's butterflies are concrete-fft's).
 *
 * A u128 word is two little-endian uint64_t (low, high); every length and row size below is in u128 words.
 * Shapes: polynomial_size in {256, 512, 1024, 2048}, glwe_dimension in {1, 2, 3} with (k+1) N <= 4096,
 * 1 <= pbs_level <= 4, 2 <= pbs_base_log <= 31, pbs_base_log * pbs_level < 128, any lwe_dimension >= 1;
 * ciphertext_modulus_log m in [65, 128], 128 = the native modulus; for m < 128 every accumulator word is
 * rounded to its m most significant bits after the last CMUX (fft128/crypto/bootstrap.rs:321-334).
 * Everything else fails with rc 1 and a message naming the limit.
 *
 * tfhe_mi355_context_create_u128 validates the parameters against these limits instead of the u64
 * kernels' (the ks_* and *_modulus fields are not read); such a context serves the _u128 calls only.  An
 * ordinary context whose shape is also within these limits takes a u128 key too.  A context holds keys of
 * ONE torus width: a _u128 upload onto a context that holds u64 or u32 keys, a u64 or u32 upload onto one
 * that holds a u128 key, and a compute call of another width than the context's keys all fail with rc 1.
 * Single-device only (a multi-device context is refused, rc 1), not coalesced, no keyswitch.  The _async
 * forms take device pointers (16-byte aligned) and the caller's stream, allocate nothing and do not
 * synchronise; scratch comes from the caller (the *_scratch query; too little is an error).  count = 0 is a
 * no-op. */
int tfhe_mi355_context_create_u128(const TfheMi355Parameters *params, int device, TfheMi355Context **out_ctx);
/* Standard u128 bootstrapping key [n][pbs_level][k+1][k+1][N] (host), converted on the device to four f64
 * planes (re.hi, re.lo, im.hi, im.lo) of N/2 entries per polynomial, in the transform's output order. */
int tfhe_mi355_bootstrap_key_upload_u128(TfheMi355Context *ctx, const uint64_t *bsk, size_t len);
/* lwe_in count x (n+1), lwe_out count x (kN+1), luts lut_count general GLWE accumulators of (k+1)N words,
 * lut_indexes one per ciphertext or NULL (all LUT 0). */
int tfhe_mi355_programmable_bootstrap_u128(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *lwe_out,
                                           const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes,
                                           size_t count, uint32_t ciphertext_modulus_log);
int tfhe_mi355_programmable_bootstrap_u128_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint64_t *d_lwe_out,
                                                 const uint64_t *d_luts, size_t lut_count,
                                                 const uint32_t *d_lut_indexes, size_t count,
                                                 uint32_t ciphertext_modulus_log, void *d_scratch,
                                                 size_t scratch_bytes, void *stream);
int tfhe_mi355_programmable_bootstrap_u128_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);
/* The same blind rotation without the sample extraction: glwe_out count x (k+1)N
 * (Fourier128LweBootstrapKey::blind_rotate_assign, bootstrap.rs:245-337). */
int tfhe_mi355_blind_rotate_u128(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out,
                                 const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count,
                                 uint32_t ciphertext_modulus_log);
int tfhe_mi355_blind_rotate_u128_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint64_t *d_glwe_out,
                                       const uint64_t *d_luts, size_t lut_count, const uint32_t *d_lut_indexes,
                                       size_t count, uint32_t ciphertext_modulus_log, void *d_scratch,
                                       size_t scratch_bytes, void *stream);
int tfhe_mi355_blind_rotate_u128_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes);
/* Diagnostic (host only, no GPU): the canonical double-double tables of the f128 FFT.  twist: 4 planes of
 * N/2 doubles (cos.hi, cos.lo, sin.hi, sin.lo of pi j / N); twiddles: 4 planes of N/4 doubles
 * (exp(-2 pi i t / (N/2))).  Every entry is hi = RN(x), lo = RN(x - hi) of the exact real x. */
int tfhe_mi355_debug_fft128_tables(uint32_t polynomial_size, double *twist, double *twiddles);
/* Diagnostic (test hook, host buffers, synchronous): the f128 kernel's backward conversion alone
 * (u128_from_torus_f128, mod.rs:226-239), one thread per value: out[i] = acc[i] + X_i (acc may be NULL),
 * X_i = floor((x - floor x) 2^128 + 1/2) mod 2^128 of the double-double x = hi[i] + lo[i]. */
int tfhe_mi355_debug_torus128_from_f128(int device, const double *hi, const double *lo, const uint64_t *acc,
                                        uint64_t *out, size_t count);
/* Diagnostic: ciphertexts (= workgroups) of the f128 PBS kernel of the context's shape resident at once. */
int tfhe_mi355_debug_pbs_u128_resident(TfheMi355Context *ctx, size_t *count);

/* ---- client-side helpers (not on the PBS path; seeded, deterministic per (seed, index)) ----
 * Binary secret keys, Gaussian noise (commons/math/random/gaussian.rs:15-52), GGSW/BSK
 * (ggsw_encryption.rs:116-150,300-331), KSK (lwe_keyswitch_key_generation.rs:60-135),
 * LWE encryption/decryption (lwe_encryption.rs).  The randomness is a seeded xoshiro256**,
 * not the reference's AES-CTR CSPRNG: use the Rust client for production keys. */
int tfhe_mi355_client_gen_binary_key(uint64_t seed, uint64_t stream, uint64_t *key, size_t len);
int tfhe_mi355_client_gen_bootstrap_key(uint64_t seed, const uint64_t *lwe_sk, uint32_t n,
                                        const uint64_t *glwe_sk, uint32_t k, uint32_t N,
                                        uint32_t base_log, uint32_t level, double std_dev,
                                        uint64_t *bsk, uint32_t threads);
/* multi-bit BSK [n/g][2^g][L][k+1][k+1][N] (lwe_multi_bit_bootstrap_key_generation.rs:87-173) */
int tfhe_mi355_client_gen_multi_bit_bootstrap_key(uint64_t seed, const uint64_t *lwe_sk, uint32_t n,
                                                  const uint64_t *glwe_sk, uint32_t k, uint32_t N,
                                                  uint32_t base_log, uint32_t level, uint32_t grouping_factor,
                                                  double std_dev, uint64_t *bsk, uint32_t threads);
int tfhe_mi355_client_gen_keyswitch_key(uint64_t seed, const uint64_t *in_sk, uint32_t in_dim,
                                        const uint64_t *out_sk, uint32_t out_dim, uint32_t base_log,
                                        uint32_t level, double std_dev, uint64_t *ksk);
/* packing KSK [in_dim][level][(k+1)N] (lwe_packing_keyswitch_key_generation.rs:74-149) */
int tfhe_mi355_client_gen_packing_keyswitch_key(uint64_t seed, const uint64_t *in_sk, uint32_t in_dim,
                                                const uint64_t *glwe_sk, uint32_t k, uint32_t N,
                                                uint32_t base_log, uint32_t level, double std_dev,
                                                uint64_t *pksk, uint32_t threads);
/* relinearisation key [k(k+1)/2][level][(k+1)N], level L first (custom_relinearization_key_generation.rs:72-161):
 * block n = i(i+1)/2 + j (j <= i), level lvl encrypts (S_i * S_j) << (64 - base_log*lvl) under glwe_sk */
int tfhe_mi355_client_gen_relinearization_key(uint64_t seed, const uint64_t *glwe_sk, uint32_t k, uint32_t N,
                                              uint32_t base_log, uint32_t level, double std_dev, uint64_t *rlk);
/* pfpksk list of the circuit bootstrap [k+1][in_dim+1][level][(k+1)N], level 1 first (lwe_wopbs.rs:80-158):
 * key g, block i, level lvl encrypts -s_i * P_g * 2^(64 - base_log*lvl); s_(in_dim) = -1 (the body),
 * P_g = polynomial g of the GLWE key (g < k) or the constant -1 (g = k) */
int tfhe_mi355_client_gen_pfpksk_list(uint64_t seed, const uint64_t *in_sk, uint32_t in_dim, const uint64_t *glwe_sk,
                                      uint32_t k, uint32_t N, uint32_t base_log, uint32_t level, double std_dev,
                                      uint64_t *pfpksk, uint32_t threads);
/* seeded keys (masks from the AES-CTR stream of mask_seed, noise from noise_seed); bodies only */
int tfhe_mi355_client_gen_seeded_bootstrap_key(uint64_t noise_seed, uint64_t mask_seed_lo, uint64_t mask_seed_hi,
                                               const uint64_t *lwe_sk, uint32_t n, const uint64_t *glwe_sk,
                                               uint32_t k, uint32_t N, uint32_t base_log, uint32_t level,
                                               double std_dev, uint64_t *bodies, uint32_t threads);
int tfhe_mi355_client_gen_seeded_keyswitch_key(uint64_t noise_seed, uint64_t mask_seed_lo, uint64_t mask_seed_hi,
                                               const uint64_t *in_sk, uint32_t in_dim, const uint64_t *out_sk,
                                               uint32_t out_dim, uint32_t base_log, uint32_t level, double std_dev,
                                               uint64_t *bodies);
int tfhe_mi355_client_csprng_mask_words(uint64_t seed_lo, uint64_t seed_hi, uint64_t first_word, size_t count,
                                        uint64_t *out);
/* compact public key [2n] = mask, body (generate_lwe_compact_public_key, lwe_compact_public_key_generation.rs:
 * 15-54): body = mask (*) reverse(sk) + noise in Z[X]/(X^n + 1) */
int tfhe_mi355_client_gen_compact_public_key(uint64_t seed, const uint64_t *sk, uint32_t n, double std_dev,
                                             uint64_t *pk);
/* compact list container, ceil(count / n) n + count words
 * (encrypt_lwe_compact_ciphertext_list_with_compact_public_key, lwe_encryption.rs:1837-2043) */
int tfhe_mi355_client_compact_encrypt(uint64_t seed, const uint64_t *pk, uint32_t n, const uint64_t *plaintexts,
                                      size_t count, double mask_std_dev, double body_std_dev, uint64_t *list);
/* seeded ciphertexts: the bodies under masks from the AES-CTR stream -- one seed each, seeds [count]{lo, hi}
 * (encrypt_seeded_lwe_ciphertext, lwe_encryption.rs:1415-1585), or one seed for the list
 * (encrypt_seeded_lwe_ciphertext_list, :1096-1253) */
int tfhe_mi355_client_seeded_lwe_encrypt(uint64_t noise_seed, const uint64_t *seeds, const uint64_t *sk, uint32_t n,
                                         const uint64_t *plaintexts, size_t count, double std_dev, uint64_t *bodies);
int tfhe_mi355_client_seeded_lwe_encrypt_list(uint64_t noise_seed, uint64_t mask_seed_lo, uint64_t mask_seed_hi,
                                              const uint64_t *sk, uint32_t n, const uint64_t *plaintexts, size_t count,
                                              double std_dev, uint64_t *bodies);
int tfhe_mi355_client_lwe_encrypt(uint64_t seed, const uint64_t *sk, uint32_t n, const uint64_t *plaintexts,
                                  size_t count, double std_dev, uint64_t *cts);
int tfhe_mi355_client_lwe_decrypt(const uint64_t *sk, uint32_t n, const uint64_t *cts, size_t count,
                                  uint64_t *plaintexts);

#ifdef __cplusplus
}
#endif

#endif /* TFHE_MI355_H */
