/*
 * zkhip.h -- C ABI of libzkhip.so, the MI355X (gfx950) Groth16 proving backend for ethsnarks.
 *
 * Drop-in boundary for the reference's proving path (citations into zkh2018/ethsnarks):
 *
 *   zk_pk_load_raw      <- ethsnarks::load_proving_key(pk_file)              src/stubs.cpp:36-39
 *                          loadFromFile<ProvingKeyT>                         src/utils.hpp:176-185
 *                          operator>>(istream&, pk_nozk&)                    r1cs_gg_ppzksnark_zok.tcc:124-143
 *   zk_pk_save_raw      <- writeToFile<ProvingKeyT> / operator<<             src/utils.hpp:166-173, tcc:108-122
 *   zk_pk_from_bellman_json / zk_pk_bellman2ethsnarks <- pk_bellman2ethsnarks + readG1/readG2   src/export.cpp:223-328
 *   zk_pk_alt2mcl / zk_pk_mcl2nozk <- pk_alt2mcl / pk_mcl2nozk                src/export.cpp:330-408
 *   zk_pk_from_parts    <- r1cs_gg_ppzksnark_zok_proving_key_nozk ctor       r1cs_gg_ppzksnark_zok.hpp:171-233
 *   zk_ctx_create       <- ProverContext<ppT>(pk) + get_domain(pb, pk, cfg)  hpp:279-291, src/stubs.cpp:61-75
 *   zk_prove            <- r1cs_gg_ppzksnark_zok_prover(ctx, pb.values)      tcc:451-550 (via prove(), stubs.cpp:42-47)
 *   zk_proof_to_json    <- proof_to_json(proof, primary_input)               src/export.cpp:99-121
 *   zk_config           <- libsnark::Config                                   src/prover_config.hpp:8-35
 *   zk_keygen           <- r1cs_gg_ppzksnark_zok_generator + nozk conversion  tcc:277-449, hpp:209-233
 *                          (stub_genkeys_from_pb, src/stubs.cpp:77-87)
 *   zk_vk_to_json       <- vk2json                                            src/export.cpp:124-145
 *   zk_vk_from_json / zk_proof_from_json <- vk_from_json / proof_from_json   src/import.cpp:161-223
 *   zk_verify / ethsnarks_verify <- stub_verify / ethsnarks_verify          src/stubs.cpp:16-33, src/verify_dll.cpp:3-10
 *
 * Plain C types only.  Field elements are 4 x u64 little-endian limbs; "Montgomery" means the
 * libff::Fp_model<4> in-memory form (value * 2^256 mod p), which is what `pb.values` and the `.raw`
 * key file contain.  Affine G1 = {x, y} (8 u64), affine G2 = {x.c0, x.c1, y.c0, y.c1} (16 u64); an
 * all-zero point encodes infinity.  All functions return 0 (ZK_OK) or a positive error code; none
 * throws or aborts.  zk_last_error() gives a thread-local human-readable message.
 *
 * There is NO CPU implementation behind this ABI: every compute entry point needs a HIP device and
 * fails with ZK_ERR_NODEVICE / ZK_ERR_HIP otherwise.
 */
#ifndef ZKHIP_H
#define ZKHIP_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ZK_OK 0
#define ZK_ERR_ARG 1       /* null / inconsistent argument */
#define ZK_ERR_IO 2        /* cannot open / read / write file (reference: assert in utils.hpp:180) */
#define ZK_ERR_FORMAT 3    /* malformed .raw stream */
#define ZK_ERR_HIP 4       /* HIP runtime error */
#define ZK_ERR_NOMEM 5
#define ZK_ERR_SHAPE 6     /* key does not match the constraint system (DEBUG asserts tcc:477-483) */
#define ZK_ERR_DEGREE 7    /* H has wrong degree: witness does not satisfy the R1CS (asserts tcc:472-474) */
#define ZK_ERR_NODEVICE 8
#define ZK_ERR_BUFFER 9    /* output buffer too small */
#define ZK_ERR_INTERNAL 10 /* an exception other than an allocation failure reached the C ABI's barrier (text in zk_last_error) */

#define ZK_CODEC_ALT_BN128 0   /* upstream libff alt_bn128 stream layout */
#define ZK_CODEC_MCL_BN128 1   /* the reference's default curve build (CMakeLists.txt:47-54); its element encoding lives in the
                                  absent libff fork and is INFERRED (same flag + raw Montgomery coordinates as ALT_BN128):
                                  parity unpinned -- the reference holds no key file (open risk).
                                  TODAY THE TWO CODEC VALUES READ AND WRITE BYTE-IDENTICAL FILES: the value is validated and
                                  recorded, nothing else; a verified mcl layout would change the point reader / writer only */

/* ABI version of this header: bumped whenever a struct below changes layout or a function changes signature.
 * 3: zk_config = {multi_exp_c, device, shard_rank, shard_count, max_batch, schedule} (24 bytes; rounds 1-2 had 16 / 24).
 * 4: the Poseidon entry points (zk_poseidon_*, zk_mtree_create_ex, zk_mtree_info); zk_mtree_paths returns width - 1 siblings per level.
 * 5: Baby JubJub (zk_jj_*, zk_pedersen_*, zk_eddsa_*).
 * 6: zk_mtree_fill_full_witnesses.
 * 7: zk_wplan_probe_program.
 * 8: zk_eddsa_fill_witnesses and zk_eddsa_layout.
 * 9: zk_eddsa_fill_pure_witnesses and zk_eddsa_pure_layout.
 *    (zk_eddsa_sign_batch and zk_eddsa_sign_probe came later WITHOUT a bump: no struct changed layout and no function changed signature.  A
 *    client that needs the signer detects it by its symbol.  zk_eddsa_fill_hash_witnesses and zk_eddsa_hash_layout came the same way: a new
 *    function and a new struct beside the old ones, detected by the symbol.  zk_eddsa_fill_witnesses_wide likewise: a new function beside
 *    zk_eddsa_fill_witnesses, which keeps its signature; a client that wants several lanes per witness detects it by the symbol.
 *    zk_mtree_update_seq and zk_mtree_update_layout likewise: new beside the old ones, detected by the symbol.  The test probes
 *    zk_ctx_probe_rows, zk_msm_sort_probe, zk_msm_stage_probe, zk_ntt_probe and zk_ctx_probe_h likewise.)
 * A client checks zk_abi_version() == ZK_ABI_VERSION once after loading the library, or passes the size of the zk_config
 * it was compiled with to zk_ctx_create_sized (members it does not know read as 0 = their defaults). */
#define ZK_ABI_VERSION 9

typedef struct zk_pk zk_pk;
typedef struct zk_vk zk_vk;
typedef struct zk_ctx zk_ctx;
typedef struct zk_wplan zk_wplan;
typedef struct zk_vctx zk_vctx;

typedef struct {
    uint32_t n_rows;
    const uint32_t *row_ptr;   /* n_rows + 1 */
    const uint32_t *col;       /* variable index; 0 is the constant ONE */
    const uint64_t *coeff;     /* nnz x 4, Montgomery Fr */
} zk_csr;

/* mirrors libsnark::Config (src/prover_config.hpp:8-35).  CPU-cache knobs of the reference
 * (num_threads, smt, fft, radixes, prefetch_*, look_ahead) have no meaning on the GPU and are
 * accepted and ignored by the C++ adapter; what remains: */
typedef struct {
    uint32_t multi_exp_c;      /* Pippenger window bits, 0 = auto (Config::multi_exp_c) */
    uint32_t device;           /* HIP device ordinal */
    uint32_t shard_rank;       /* MSM base-range sharding: this context owns shard_rank of shard_count */
    uint32_t shard_count;      /* 0 or 1 = unsharded */
    uint32_t max_batch;        /* proofs of this circuit one launch sequence may carry (zk_prove_batch); 0 or 1 = one at a time */
    uint32_t schedule;         /* ZK_SCHED_OVERLAP (0): the proof's sorts, accumulations and reduction tails on five streams --
                                * lowest latency of one proof, what large circuits want; ZK_SCHED_ONE_STREAM (1): every launch on one
                                * stream -- for many small proofs in many contexts (a hardware queue runs its dispatches in order, so
                                * fewer streams per context leave more queues to other contexts: profiles/r02_small_circuit_concurrency.txt);
                                * ZK_SCHED_LATENCY (2): ZK_SCHED_OVERLAP for a context that proves ONE synchronous proof at a time (zk_prove =
                                * ethsnarks::prove): its streams share one priority, which shortens a lone proof of 2^16 constraints and more
                                * by 3-19 % and costs pipelined contexts 10 % (profiles/r03_queue_mapping.txt) */
} zk_config;
#define ZK_SCHED_OVERLAP 0
#define ZK_SCHED_ONE_STREAM 1
#define ZK_SCHED_LATENCY 2

/* canonical (non-Montgomery) affine coordinates; *_inf != 0 => point at infinity, printed as (0, 1) */
typedef struct {
    uint64_t a_x[4], a_y[4];
    uint64_t b_x_c0[4], b_x_c1[4], b_y_c0[4], b_y_c1[4];
    uint64_t c_x[4], c_y[4];
    uint32_t a_inf, b_inf, c_inf, _pad;
} zk_proof;

/* per-shard partial results of the four multi-exponentiations, XYZZ coordinates, Montgomery:
 * At, Ht, Lt: 4 x 4 u64 each (G1); Bt: 4 x 8 u64 (G2)  => 3*128 + 256 = 640 bytes.
 * The proof only ever uses Ht + Lt (C = Ht + Lt, tcc:540): when the H- and the L-query share their bucket set (the usual case)
 * ONE bucket reduction serves both, Ht carries the sum and Lt the point at infinity (all zero); zk_prove_combine adds them either way. */
typedef struct {
    uint64_t At[16], Bt[32], Ht[16], Lt[16];
} zk_partials;

/* phase times in milliseconds, named after the reference's enter_block labels (tcc:460-542) */
typedef struct {
    float h2d_witness;
    float compute_h;           /* "Compute the polynomial H" */
    float a_query, b_query, h_query, l_query;   /* "Compute the proof's A-query" ... "L-query": GPU time of each multi-exponentiation */
    float gpu_total;           /* first kernel to last copy */
    float host_finish;         /* "Compute the proof": final additions (tcc:533-540), affine conversion */
    float acc_a, acc_b, acc_h, acc_l;   /* k_msm_accumulate launch of each query, HIP events on its stream */
} zk_timings;

/* ---- library / device */
const char *zk_version(void);
uint32_t zk_abi_version(void);
const char *zk_strerror(int code);
const char *zk_last_error(void);
int zk_device_count(int *count);

/* ---- proving key (host object; zk_ctx_create uploads it) */
int zk_pk_load_raw(const char *path, int codec, zk_pk **out);
int zk_pk_save_raw(const zk_pk *pk, const char *path, int codec);
/* bellman / snarkjs style proving-key JSON (keys A, B1, B2, C, hExps, vk_alfa_1, vk_beta_1/2, vk_delta_1/2; Jacobian
 * decimal triples) -> nozk key, exactly as pk_bellman2ethsnarks maps it (one public input: L = C[2..]);
 * zk_pk_bellman2ethsnarks writes the `.raw` file the reference's converter writes */
int zk_pk_from_bellman_json(const char *json_path, zk_pk **out);
int zk_pk_bellman2ethsnarks(const char *bellman_pk_json, const char *pk_raw);
/* the reference's offline converters over the FULL (zero-knowledge) proving key stream (tcc:53-90):
 * pk_alt2mcl (src/export.cpp:352-397: every coordinate goes through its decimal string) and
 * pk_mcl2nozk (src/export.cpp:399-408: nozk conversion of hpp:209-233, written with the MCL codec) */
int zk_pk_alt2mcl(const char *alt_pk_file, const char *mcl_pk_file);
int zk_pk_mcl2nozk(const char *mcl_pk_file, const char *nozk_pk_file);
/* the FULL key stream (tcc:53-90) as a proving key for zero-knowledge proofs (zk_prove_zk*):
 *   zk_pk_load_raw_full  reads it (same codec rules as full_load): the key zk_pk_mcl2nozk would make (A-query sparsified, B-query's
 *                        G2 half) plus the G1 half of the B-query (zk_pk_part 11); it proves without zero knowledge as well
 *   zk_pk_save_raw_full  writes the full stream again, the A-query re-densified over its domain; ZK_ERR_ARG for a nozk key
 *   zk_pk_is_full        1 for a key that holds the G1 half of the B-query, else 0 */
int zk_pk_load_raw_full(const char *path, int codec, zk_pk **out);
int zk_pk_save_raw_full(const zk_pk *pk, const char *path, int codec);
int zk_pk_is_full(const zk_pk *pk);
int zk_pk_from_parts(const uint64_t *alpha_g1, const uint64_t *beta_g1, const uint64_t *beta_g2,
                     const uint64_t *delta_g1, const uint64_t *delta_g2,
                     uint32_t a_domain, uint32_t nA, const uint32_t *a_idx, const uint64_t *a_val,
                     uint32_t b_domain, uint32_t nB, const uint32_t *b_idx, const uint64_t *b_val,
                     uint32_t nH, const uint64_t *H, uint32_t nL, const uint64_t *L, zk_pk **out);
/* sizes[0..5] = A.domain, nA, B.domain, nB, nH, nL */
int zk_pk_sizes(const zk_pk *pk, uint32_t sizes[6]);
/* which: 0 alpha_g1 1 beta_g1 2 beta_g2 3 delta_g1 4 delta_g2 5 A.idx 6 A.val 7 B.idx 8 B.val 9 H 10 L
 *        11 B1.val: the G1 half of the B-query (nB x 8 u64, same indices as B.val; full keys only, else empty) */
const void *zk_pk_part(const zk_pk *pk, int which);
void zk_pk_free(zk_pk *pk);

/* ---- key generation: the QAP is evaluated at t on the host, the fixed-base
 * exponentiations (A, B, H, L queries, gammaABC) run on the GPU.
 * toxic_canon = t, alpha, beta, gamma, delta as canonical 4 x u64 each (the reference draws them with
 * Fr::random_element(), tcc:283-287).  Generators: G1 (1, 2), G2 the standard alt_bn128 generator. */
int zk_keygen(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t nIn, uint32_t V,
              const uint64_t toxic_canon[20], int device, zk_pk **pk_out, zk_vk **vk_out);
/* the same key, full: it also holds B1.val[i] = Bt_i G1 (zk_pk_part 11), what zero-knowledge proofs need */
int zk_keygen_full(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t nIn, uint32_t V,
                   const uint64_t toxic_canon[20], int device, zk_pk **pk_out, zk_vk **vk_out);
int zk_vk_to_json(const zk_vk *vk, char *buf, size_t cap, size_t *len);
/* vk_from_json / proof_from_json (src/import.cpp:161-223): "0x" hex or decimal strings, Fq2 as [c1, c0].
 * zk_proof_from_json: the proof's public inputs come back canonical (4 x u64 each) in inputs_canon[0 .. *n_inputs);
 * ZK_ERR_BUFFER if cap is too small (*n_inputs still set), ZK_ERR_FORMAT on malformed text or coordinates >= q */
int zk_vk_from_json(const char *vk_json, zk_vk **out);
int zk_proof_from_json(const char *proof_json, zk_proof *out, uint64_t *inputs_canon, uint32_t cap, uint32_t *n_inputs);
void zk_vk_free(zk_vk *vk);

/* ---- prover context: uploads bases + CSR once, builds domain tables, owns all scratch.
 * Borrows nothing after return (pk and CSR may be freed), one context per concurrent prover. */
uint32_t zk_domain_size(uint32_t nC, uint32_t nIn);                      /* src/stubs.cpp:49-65 */
int zk_ctx_create(const zk_pk *pk, const zk_csr *A, const zk_csr *B, const zk_csr *C,
                  uint32_t nC, uint32_t nIn, uint32_t V, const zk_config *cfg, zk_ctx **out);
int zk_ctx_create_sized(const zk_pk *pk, const zk_csr *A, const zk_csr *B, const zk_csr *C,
                        uint32_t nC, uint32_t nIn, uint32_t V, const zk_config *cfg, size_t cfg_size, zk_ctx **out);
void zk_ctx_destroy(zk_ctx *ctx);

/* witness: (V + 1) x 4 u64, ONE at index 0 (pb.values layout), Montgomery unless canonical != 0 */
int zk_prove(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_proof *out);
int zk_prove_timed(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_proof *out, zk_timings *t);
/* sharded contexts: each rank computes its partial sums; after exchanging them (e.g. an RCCL
 * all-gather of the 640-byte structs), any rank folds them in rank order and finishes the proof */
int zk_prove_partial(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_partials *out);
int zk_prove_partial_timed(zk_ctx *ctx, const uint64_t *witness, int canonical, zk_partials *out, zk_timings *t);
int zk_prove_combine(const zk_ctx *ctx, const zk_partials *parts, uint32_t count, zk_proof *out);
/* asynchronous form of zk_prove_partial: submit enqueues the whole proof on the context's streams and returns;
 * collect waits for it.  One proof in flight per context; several contexts keep the GPU full (ProverContext is
 * per concurrent prover in the reference too, hpp:279-291). */
int zk_prove_submit(zk_ctx *ctx, const uint64_t *witness, int canonical);
int zk_prove_collect(zk_ctx *ctx, zk_partials *out, zk_timings *t);
/* sharded provers, exchange on device buffers: after zk_prove_collect_device the four partial sums sit in a 640-byte device
 * buffer owned by the context (zk_ctx_partials_device; zk_partials layout) -- the send buffer of an RCCL all-gather;
 * zk_prove_combine_device folds `count` gathered 640-byte records (device pointer) in rank order like zk_prove_combine */
const void *zk_ctx_partials_device(const zk_ctx *ctx);
int zk_prove_collect_device(zk_ctx *ctx, zk_timings *t);
int zk_prove_combine_device(const zk_ctx *ctx, const void *d_parts, uint32_t count, zk_proof *out);
/* ---- several proofs of ONE circuit per launch sequence (the reference's nearest idea is the scratch reuse of
 * ProverContext, hpp:286-289): k <= zk_config.max_batch witnesses, contiguous (k x (V + 1) x 4 u64).  The k digit streams are
 * bucket-sorted together under the key (proof, bucket) and every kernel of the prover runs once for all of them, which is what
 * small circuits need: one proof alone is ~50 launches of latency-bound kernels.  Proof p is byte-identical to zk_prove of
 * witness p.  out: k records. */
int zk_prove_batch(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, zk_proof *out);
int zk_prove_batch_submit(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical);
int zk_prove_batch_submit_resident(zk_ctx *ctx, const void *d_witnesses, uint32_t k, int canonical);
int zk_prove_batch_collect(zk_ctx *ctx, zk_partials *out, uint32_t k, zk_timings *t);
/* ---- zero-knowledge proofs (libsnark's r1cs_gg_ppzksnark_prover; upstream ethsnarks): with two random scalars r, s per proof
 *   A = alpha1 + sum w_i A_i + r delta1,  B = beta2 + sum w_i B_i + s delta2,  C = sum h_j H_j + sum_{i>nIn} w_i L_i + s A + r B1 - r s delta1
 * where B1 = beta1 + sum w_i B1_i + s delta1 uses the G1 half of the B-query.  r = s = 0 gives the zk_prove bytes; the verifier is unchanged.
 * Contexts created from a full key only (zk_pk_load_raw_full / zk_keygen_full), unsharded (ZK_ERR_ARG otherwise).  The blinding runs on the
 * device.  A zero-knowledge proof in flight is collected with zk_prove_zk_batch_collect (also for k = 1), a plain one with
 * zk_prove_collect / zk_prove_batch_collect: the other collect returns ZK_ERR_ARG.  The library clears its copies of r, s once the proof
 * is collected (or dropped) and never logs them.
 * rs_canon: per proof {r, s} as canonical 4 x u64 each (k x 8 u64), every value < the Fr modulus (else ZK_ERR_ARG);
 * NULL = drawn per proof from the operating system's CSPRNG (getrandom(2), 64 bytes reduced mod r). */
int zk_prove_zk(zk_ctx *ctx, const uint64_t *witness, int canonical, const uint64_t *rs_canon, zk_proof *out);
int zk_prove_zk_batch(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, const uint64_t *rs_canon, zk_proof *out);
int zk_prove_zk_batch_submit(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, const uint64_t *rs_canon);
int zk_prove_zk_batch_submit_resident(zk_ctx *ctx, const void *d_witnesses, uint32_t k, int canonical, const uint64_t *rs_canon);
int zk_prove_zk_batch_collect(zk_ctx *ctx, zk_proof *out, uint32_t k, zk_timings *t);
/* ---- sharded latency mode, SURVEY 8(e) option 2: the three transform chains of the witness map (row evaluations of A, B or C,
 * iFFT, cosetFFT) run on three different ranks instead of being replicated on all of them.
 *   zk_chain_submit         queue chain `which` (0 A, 1 B, 2 C) of this witness; its m results end up at zk_chain_device (A, B: evaluations on
 *                           the coset; C: coefficients divided by Z on the coset -- the witness map here needs six transforms, C never goes to the coset)
 *   zk_h_from_chains_submit queue (a b - c) / Z on the coset + icosetFFT from three chain buffers in THIS device's memory
 *                           (received from the other ranks); h ends up at zk_h_device (m elements)
 *   zk_chain_wait           wait for what was queued (check_degree: ZK_ERR_DEGREE unless h[m-1] = 0)
 *   zk_prove_submit_with_h  zk_prove_submit that takes this shard's coefficients of H -- h[lo .. hi), lo = (m-1) rank / count,
 *                           hi = (m-1) (rank+1) / count -- from a device buffer instead of computing H; collect as usual */
int zk_chain_submit(zk_ctx *ctx, const uint64_t *witness, int canonical, int which);
const void *zk_chain_device(const zk_ctx *ctx, int which);
int zk_h_from_chains_submit(zk_ctx *ctx, const void *dA, const void *dB, const void *dC);
const void *zk_h_device(const zk_ctx *ctx);
int zk_chain_wait(zk_ctx *ctx, int check_degree);
int zk_prove_submit_with_h(zk_ctx *ctx, const uint64_t *witness, int canonical, const void *d_h);
/* zk_prove_submit_with_h in two steps, so that every rank starts its witness sorts and A-, B-, L-query accumulations BEFORE H exists:
 *   zk_prove_submit_defer_h  queues everything that needs only the witness (upload, witness sorts, A-, B-, L-query);
 *                            zk_chain_submit (witness = NULL: the deferred proof's) / zk_h_from_chains_submit may follow on this context
 *   zk_prove_submit_h        queues the H-query from this shard's coefficients; collect as usual
 *   zk_prove_abort           drops a proof in flight (e.g. one that will not get its H part because rank 0 found the witness
 *                            unsatisfying): drains the context's streams, nothing is returned */
int zk_prove_submit_defer_h(zk_ctx *ctx, const uint64_t *witness, int canonical);
int zk_prove_submit_h(zk_ctx *ctx, const void *d_h);
int zk_prove_abort(zk_ctx *ctx);
/* zk_prove_submit for a witness that is already resident in the context's device memory (d_witness = device
 * pointer to (V + 1) x 32 bytes, e.g. written by a GPU witness generator); it must stay untouched until collected */
int zk_prove_submit_resident(zk_ctx *ctx, const void *d_witness, int canonical);
/* zk_prove_submit for a witness in PINNED host memory (SURVEY 8(d)'s metric: "witness already in pinned host memory"): the
 * asynchronous H2D copy reads the caller's buffer where it lies -- zk_prove_submit copies a pageable buffer into the context's
 * pinned staging buffer first, 33 MB of memcpy per proof at 2^20 --, so it must stay untouched until the proof is collected.
 * zk_host_alloc / zk_host_free: pinned host memory; zk_host_register / _unregister: pin a buffer the caller already owns
 * (pb.values of a protoboard that is proven repeatedly). */
int zk_prove_submit_pinned(zk_ctx *ctx, const uint64_t *witness, int canonical);
int zk_prove_batch_submit_pinned(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical);
int zk_host_alloc(size_t bytes, void **out);
int zk_host_free(void *p);
int zk_host_register(void *p, size_t bytes);
int zk_host_unregister(void *p);
/* double-buffered upload: zk_prove_stage copies the NEXT witness (k of them, k <= zk_config.max_batch) to the
 * device on a copy stream, also while a proof is in flight on this context; zk_prove_submit_staged starts that proof with no
 * upload on its critical path (collect as usual: zk_prove_collect / zk_prove_batch_collect).  One staged witness per context. */
int zk_prove_stage(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical);
int zk_prove_stage_pinned(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical);   /* pinned source: no staging memcpy; untouched until collected */
int zk_prove_submit_staged(zk_ctx *ctx);
/* info[3q .. 3q+2] = {window bits c, windows W, buckets 2^(c-1)} of query q = A, B, H, L; info[12..14] = the A-, B-, L-query
 * ride the shared witness sort; info[15] = domain size m */
int zk_ctx_info(const zk_ctx *ctx, uint32_t info[16]);
/* the window-multiple tables of the context's key shard: info = {bytes they take, bytes they would take with every window tabulated,
 * planes S, table rows of the B-query}.  S = 1 is the default layout (all W windows: 16 x the key).  When that does not fit the device --
 * the reference's domain goes up to 2^28, src/stubs.cpp:49-75 -- zk_ctx_create keeps every S-th window only (S = 2, 4, 8, 16) and proves
 * with S bucket planes instead of failing; the proof bytes are the same.  ZK_TABLE_BUDGET=<bytes> in the environment at context creation
 * caps the tables below the free device memory. */
int zk_ctx_table_info(const zk_ctx *ctx, uint64_t info[4]);
/* The four-transform prover: an unsharded context with full tables keeps the H-query in coset-Lagrange bases (m bases Q_j, scalars
 * A(g w^j) B(g w^j)) and the L-query over all V + 1 variables (bases L_v - K_v), built once per key AND circuit at context creation and shared
 * like the other tables; a proof then needs four transforms instead of six and has the same bytes.  ZK_SIX_TRANSFORMS=1 in the environment
 * at context creation keeps the key's own bases and the six transforms (sharded contexts and frugal tables always do).
 * info = {1 if this context proves with four transforms, microseconds the transform of the bases took when the tables were built
 *         (without their window-multiple expansion), 0, 0} */
int zk_ctx_hlagrange_info(const zk_ctx *ctx, uint64_t info[4]);
/* test entry points of that transform.  Points are affine, 8 x u64 each (x, y: Montgomery Fq), (0, 0) = the point at infinity.
 * zk_hl_probe_dft:     out[j] = 1 / (m Z(g)) sum_{i < n} r^(-i) w^(-ij) points[i], j < m = 2^logm, r = g (coset != 0) or 1
 * zk_hl_probe_columns: out[v] = L_v - sum_j C[j][v] lambda[j], v <= V; L_v = l_bases[v - nIn - 1], the point at infinity for v <= nIn */
int zk_hl_probe_dft(const uint64_t *points, uint32_t n, uint32_t logm, int coset, int device, uint64_t *out);
int zk_hl_probe_columns(const zk_csr *C, uint32_t nIn, uint32_t V, const uint64_t *lambda, uint32_t m, const uint64_t *l_bases, int device, uint64_t *out);
/* row probe: TEST INFRASTRUCTURE.  Uploads the k witnesses (contiguous, V + 1 elements each) as a batch submit does, runs the R1CS row
 * evaluation that every H pipeline starts with -- the same helper, the same arguments -- and copies back what the row kernels left:
 * out = [A: k x m][B: k x m][C: k x m], m = the domain size, 4 x u64 per element, RAW Montgomery limbs (no canon), rows nC .. m - 1 (A's
 * input-consistency rows and the padding) included.  ZK_ERR_ARG: a proof is in flight, k = 0, k > zk_config.max_batch.  (A new function
 * WITHOUT an ABI bump: detected by its symbol.) */
int zk_ctx_probe_rows(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, uint64_t *out /* 3 x k x m x 4 */);
/* sort probe: TEST INFRASTRUCTURE.  The bucket sort in front of every multi-exponentiation, alone: a sort-only work object (no table, no
 * curve arithmetic) sized for exactly this call, one sort of `batch` scalar vectors of n elements each (proof p reads
 * scalars[(p * stride + i) * 4 ..], stride >= n; Montgomery unless canonical), and what the last sort kernel left.
 *   c: window bits, 0 = the library's choice for (n, batch), clamped to 2 .. 20;  plog: 2^plog bucket planes (frugal tables), <= 7;
 *   shift_payload != 0: entries carry (row << kbits) | i as the shared witness sort of a context does, else row * n + i; the sign is bit 31.
 *   off[0 .. nb_total]: entries before each bucket, nb_total = batch * 2^plog * 2^(c-1); bucket id = ((p << plog) | (w mod 2^plog)) * 2^(c-1)
 *                       + |digit| - 1 for window w of proof p, row = w >> plog.  off_cap (in words) must be >= nb_total + 1.
 *   sorted[0 .. off[nb_total]): the entries, bucket after bucket; the order INSIDE a bucket is not defined.
 *   info = {c, W, nb_total, cb, fb, fine_bits, groups, per_group, kbits (0: row * n + i), 1 if the staged partition ran / 0 the direct
 *           scatter, off[nb_total], 0 ...}: the window and sort shape actually used (ZK_SORT_PER_GROUP in the environment is read as the
 *           proving path reads it).
 * ZK_ERR_ARG: a null pointer (scalars may be null for n = 0), batch = 0, stride < n, plog > 7, more than 2^20 buckets ("batch too large"),
 * off_cap too small, sorted_cap (in words) below off[nb_total] -- info is filled in that case, sorted is not written.  (A new function
 * WITHOUT an ABI bump: detected by its symbol.) */
int zk_msm_sort_probe(const uint64_t *scalars, uint32_t n, uint32_t batch, uint32_t stride, int canonical, uint32_t c, uint32_t plog,
                      int shift_payload, int device, uint32_t *off, uint64_t off_cap, uint32_t *sorted, uint64_t sorted_cap, uint32_t info[16]);
/* stage probe: TEST INFRASTRUCTURE.  ONE multi-exponentiation on the default stream through the members a context drives (MsmWork::alloc,
 * precompute, enqueue_sort, enqueue_accumulate, enqueue_tail), a synchronisation, and what every stage left in the work buffers: RAW device
 * values (loose domain, no canon).  No kernel and no launch code knows about the probe.
 * One MSM (zk_msm_stage_in): n bases (affine, 8 / 16 x u64, Montgomery, (0, 0) = infinity) and its scalars (4 x u64, Montgomery unless
 * canonical).  n_src = 0: the MSM sorts its own n scalars.  n_src != 0, the BORROWED sort: a sort-only work sorts n_src scalars (with
 * (row << kbits) | i entries if shift_payload != 0, as the shared witness sort of a context does) and the MSM's n <= n_src bases are driven
 * through view_for(offset, pos): scalar i belongs to base pos[i] (0xffffffff or >= n: absent) or, pos = NULL, to base i - offset.
 * `second` (optional; own sort only): another MSM with the same c, plog and bucket count whose chunk pieces are folded into the first one's
 * bucket reduction (enqueue_tail's `also`), as the H- and the L-query of a proof are.
 *   c: window bits, 0 = the library's choice, clamped to 2 .. 20;  plog: 2^plog bucket planes, <= 7;  tail_lanes: 0 (the shape's) / 1 / 4.
 *   ZK_MSM_QUAD, ZK_MSM_QUAD_ACC, ZK_ACC_PAIRS, ZK_ROWCOL_SEG, ZK_SEG_MIN and ZK_SEG_MAX in the environment are read as the proving path
 *   reads them.
 * Outputs (zk_msm_stage_out; every capacity counts elements of the pointer's type and is checked BEFORE anything is launched; AW = 8 / 16
 * and XW = 16 / 32 u64 per affine / XYZZ point of G1 / G2; sets = 2^plog, nbt = sets * 2^(c-1), n_sort = n_src ? n_src : n):
 *   table      rows x n affine points, rows = ceil(W / sets)                       cap >= rows * n * AW
 *   off        nbt + 1 words;  sorted: off[nbt] words                              cap >= nbt + 1;  cap >= n_sort * W
 *   pieces     info[20] XYZZ points: piece index 0 .. chunks + nbt - 2.  Slots outside every bucket's piece range were never written and
 *              hold the probe's fill pattern (all bits set), as do all of pieces, bucket, partial_a and partial_b before the launches
 *                                                                                  cap >= (min(n_sort W / seg_max + slots + 1, ceil(n_sort W / seg_min)) + nbt) * XW
 *   heavy_list info[21] words (heavy_count), in the order the device queued them   cap >= nbt
 *   bucket     nbt XYZZ points;  partial_a: sets x (H + L) XYZZ points, H = 2^hi_bits row sums then L = 2^lo_bits column sums per set;
 *              partial_b: sets XYZZ points;  result: finish() + to_affine, one affine point
 *   off2 / sorted2 / pieces2: the second MSM's, same rules with its n (only read when `second` is given)
 *   info = {c, W, 2^(c-1), plog, sets, lo_bits, hi_bits, quad, quad_acc, acc_pairs, accumulation kernel lanes form (1 / 2 / 4), rowcol_seg,
 *           chunk.slots, seg_min, seg_max, entries = off[nbt], MSM_HEAVY, MSM_TREE, lanes the tail ran with, rows, pieces copied, heavy_count,
 *           kbits of the borrowed sort, 1 if a second MSM was folded in, then slots, seg_min, seg_max, entries, accumulation form and pieces
 *           copied of the second MSM, MSM_HEAVY_GRID, 0}
 * ZK_ERR_ARG (nothing launched): a null pointer, n = 0, a capacity too small, plog > 7, a borrowed sort with n > n_src, with pos = NULL and
 * offset + n > n_src, or with a pos[i] that is neither 0xffffffff nor below n; a second MSM with n_src != 0 or, from the work objects,
 * with other buckets.  ZK_ERR_INTERNAL: heavy_count or off[nbt] exceed their buffers -- nothing past an allocation is read back.  (A new
 * function WITHOUT an ABI bump: detected by its symbol.) */
typedef struct zk_msm_stage_in {
    const uint64_t *bases, *scalars;
    const uint32_t *pos;            /* n_src words or NULL */
    uint32_t n, n_src, offset;
    int shift_payload;
} zk_msm_stage_in;
typedef struct zk_msm_stage_out {
    uint64_t *table, *pieces, *bucket, *partial_a, *partial_b, *result, *pieces2;
    uint32_t *off, *sorted, *heavy_list, *off2, *sorted2;
    uint64_t table_cap, pieces_cap, bucket_cap, partial_a_cap, partial_b_cap, result_cap, pieces2_cap;
    uint64_t off_cap, sorted_cap, heavy_cap, off2_cap, sorted2_cap;
    uint32_t info[32];
} zk_msm_stage_out;
int zk_msm_stage_probe(int g2, const zk_msm_stage_in *first, const zk_msm_stage_in *second, int canonical, uint32_t c, uint32_t plog,
                       uint32_t tail_lanes, int device, zk_msm_stage_out *out);
/* transform probe: TEST INFRASTRUCTURE.  Builds the production scaling and twiddle tables for m = 2^logm, uploads the caller's arrays, calls
 * the transform driver (csrc/ntt.hpp ntt_run) ONCE with the batch, stride and fused steps a proof gives it, synchronises and copies the output
 * back.  zk_ntt is the case batch = 1, stride = 0, nothing fused.
 *   in, out, in2, sub: batch x stride elements each (4 x u64, RAW words as the kernels read and leave them: Montgomery in every production
 *     call; the loose representatives [0, 2r) are accepted on input as by the butterflies).  Vector v lies at element v * stride; stride >= m.
 *     Every array is copied WHOLE, the stride - m words behind each vector included: `out` is uploaded before the call and downloaded after
 *     it, so whatever the caller left in the gaps of `out` comes back unless a kernel wrote there.
 *   inverse: the inverse twiddles (no 1 / m by itself: that is a post table).  pre: 0 none, 1 coset_fwd (g^i).
 *   post, post_alt: 0 none, 1 inv_m (1 / m), 2 icoset (g^-i / m), 3 inv_then_coset (g^i / m), 4 inv_m_zinv (1 / (m Z(g))),
 *     5 icoset_zinv (g^-i / (m Z(g)));  g = 5, Z(g) = g^m - 1.  Vectors v >= alt_from are scaled by post_alt (if not 0) instead of post.
 *   in2 (or NULL): the transform's input is in[i] * in2[i] (Montgomery product).  sub (or NULL): out[i] = v * post[i] - sub[i].
 *   Output words: a scaled vector is the strict Montgomery product, canonical [0, r); an unscaled one is reduced to [0, r) by the last pass.
 * ZK_ERR_ARG, nothing launched and `out` not written: in or out NULL, logm > 28, batch = 0, stride < m, a table number out of range, sub
 * without post.  (A new function WITHOUT an ABI bump: detected by its symbol.) */
int zk_ntt_probe(const uint64_t *in, const uint64_t *in2, const uint64_t *sub, uint64_t *out, uint32_t logm, uint32_t batch, uint32_t stride,
                 int inverse, int pre, int post, int post_alt, uint32_t alt_from, int device);
/* H probe: TEST INFRASTRUCTURE.  Uploads the k witnesses as zk_ctx_probe_rows does and runs the context's OWN H pipeline on its main stream --
 * the six-transform one, or the four-transform one when the context keeps the H-query in coset-Lagrange bases -- with device-to-host copies
 * enqueued between its launches.  The kernels, their arguments and their order are those of a proof; a proof passes no snapshot buffers.
 * All outputs are RAW device words, 4 x u64 per element, vector p of a group at element p * m.  R = 2^256 mod r; "Montgomery" = value * R.
 *   first   after the first transform.  six: [A: k][B: k][C: k] x m -- a_i g^i, b_i g^i (coefficients of the interpolants times the coset
 *           shift) and c_i / Z(g), Montgomery.  four: [A: k][B: k] x m -- a_i g^i Montgomery, b_i g^i CANONICAL (the post-scale of B carries
 *           1 / R); the third group of `first` is not written.  The caller gives 3 k m elements either way.
 *   coset   after the second transform: [A: k][B: k] x m, A(g w^j) and B(g w^j) in the representations above, reduced to [0, r).
 *   last    six: h, k x m, Montgomery, h = (icosetFFT(A B) - C) / Z(g), coefficient m - 1 included.  four: p_j = A(g w^j) B(g w^j), k x m,
 *           CANONICAL (the H scalars as the bucket sort reads them).
 *   hpart   four only: 2 x grid x k elements; pair (2 (p grid + x), + 1) is workgroup x's share of proof p's degree check, over j in
 *           [2048 x, 2048 (x + 1)): sum_j w^j p_j CANONICAL, then sum_j w^j c_j Montgomery (c_j = the C row evaluations).  grid = ceil(m / 2048).
 *   tail    four only: k elements, h[m-1] of every proof, Montgomery:  (g^-(m-1) sum_j w^j p_j - sum_j w^j c_j) / (m Z(g)).
 *   h_tail  k elements, always: the pinned words the degree check of a proof reads (Montgomery h[m-1]; zero iff the witness satisfies).
 *   info = {1 four transforms / 0 six, m, k, grid of k_hl_product (0 with six transforms), 0, 0, 0, 0}
 * ZK_ERR_ARG, nothing written to any output: a null pointer (hpart and tail must be given even with six transforms, where they stay
 * unwritten), a proof in flight, k = 0, k > zk_config.max_batch.  (A new function WITHOUT an ABI bump: detected by its symbol.) */
int zk_ctx_probe_h(zk_ctx *ctx, const uint64_t *witnesses, uint32_t k, int canonical, uint64_t *first /* 3 k m x 4 */, uint64_t *coset /* 2 k m x 4 */,
                   uint64_t *last /* k m x 4 */, uint64_t *hpart /* 2 grid k x 4 */, uint64_t *tail /* k x 4 */, uint64_t *h_tail /* k x 4 */, uint32_t info[8]);

/* inputs: nIn Fr elements = witness[1..nIn] (Montgomery unless canonical); returns the JSON length
 * (excluding NUL) through *len; ZK_ERR_BUFFER if cap is too small (len still set) */
int zk_proof_to_json(const zk_proof *proof, const uint64_t *inputs, uint32_t nIn, int canonical,
                     char *buf, size_t cap, size_t *len);

/* ---- verifier (host code, as in the reference): r1cs_gg_ppzksnark_zok_verifier_strong_IC
 * (tcc:552-670) behind stub_verify (src/stubs.cpp:16-33).  *accepted = 1 iff the proof verifies. */
int zk_verify(const char *vk_json, const char *proof_json, int *accepted);
/* same symbol and signature as the reference's libethsnarks_verify (src/verify_dll.cpp:3-10) */
bool ethsnarks_verify(const char *vk_json, const char *proof_json);
/* ---- batch verifier on the device: k proofs of ONE key per call, the pairing work in HIP kernels (csrc/pairing.hpp, verify_gpu.cpp).
 * zk_vctx_create uploads the key once: window tables of gammaABC[1..], line tables of gamma and delta, e(alpha, beta), staging for
 * max_batch (1 .. 2^20) proofs; a key with a point off its curve is ZK_ERR_FORMAT.  The verdict of every proof equals zk_verify's on
 * the text zk_proof_to_json writes for it (the coordinates; the *_inf flags are not read): an all-zero point is infinity and enters the
 * product as 1, the (0, 1) the prover writes for an infinite point is on neither curve and is rejected, as are coordinates >= q, inputs >= r, points off their curves and B outside the order-r subgroup.
 * A rejected proof does not disturb its neighbours.  One batch at a time per context (calls on one context are serialised).
 *   proofs: k records; inputs_canon: k x nIn x 4 u64 canonical, nIn = |gammaABC| - 1 (may be NULL when nIn = 0);
 *   accepted: k bytes, 1 = verifies.  ZK_ERR_ARG for null arguments, k = 0, k > max_batch. */
int zk_vctx_create(const zk_vk *vk, int device, uint32_t max_batch, zk_vctx **out);
void zk_vctx_destroy(zk_vctx *v);
int zk_verify_batch(zk_vctx *v, const zk_proof *proofs, const uint64_t *inputs_canon, uint32_t k, uint8_t *accepted);
/* the same from k proof_to_json texts; a text that does not parse or has the wrong number of inputs gets 0 */
int zk_verify_batch_json(zk_vctx *v, const char *const *proof_json, uint32_t k, uint8_t *accepted);

/* ---- witness completion on the GPU (the reference fills pb.values on the host, gadget by gadget).  For a
 * constraint system in "solved order" -- every constraint reads known variables in A and B and introduces at most one new
 * variable, linearly, in C (the MiMC / Merkle gadgets, the synthetic chain) -- the system itself is the witness program.
 *   zk_wplan_create  compiles it; known[v] != 0 marks the variables the caller will supply (V + 1 flags; ONE is implied);
 *                    ZK_ERR_ARG with an explanatory message when the constraints are not in solved order
 *   zk_wplan_solve   completes k witnesses in place: d_w = device pointer to k x (V + 1) Fr elements (Montgomery), supplied
 *                    variables filled in; *violations = constraints that introduce nothing and do not hold (0 = all satisfied).
 *                    The buffer can go straight to zk_prove_batch_submit_resident: the witnesses never visit the host.
 * zk_dev_*: device-memory helpers for hosts without a HIP binding of their own. */
int zk_wplan_create(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t V, const uint8_t *known, int device, zk_wplan **out);
/* ... with HINTS for values the constraints only check (gadgets with non-deterministic advice, e.g. src/gadgets/field2bits_strict.cpp):
 *   ZK_WHINT_BITS      w[first + i] = bit i of the canonical value of w[src], i < count
 *   ZK_WHINT_INV       w[first] = 1 / w[src], 0 when w[src] = 0            (count = 1; src/gadgets/isnonzero.cpp: M)
 *   ZK_WHINT_NONZERO   w[first] = 1 when w[src] != 0, else 0               (count = 1; src/gadgets/isnonzero.cpp: Y)
 * A hint runs right before the first constraint that reads one of its variables (its source must be known by then). */
#define ZK_WHINT_BITS 1
#define ZK_WHINT_INV 2
#define ZK_WHINT_NONZERO 3
typedef struct { uint32_t kind, src, first, count; } zk_whint;
int zk_wplan_create_hinted(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t V, const uint8_t *known,
                           const zk_whint *hints, uint32_t n_hints, int device, zk_wplan **out);
/* ... as a WIDE plan: `lanes` lanes (a power of two, 4 .. 64; a wave holds 64 / lanes witnesses) work on ONE witness.  Same semantics, same
 * refusals and messages as zk_wplan_create_hinted (n_hints = 0 with hints = NULL is the hint-free form): the constraints are classified in the
 * given order by the same rule, so the completed rows are byte-identical and the violation counts equal.  Each linear combination becomes
 * chunked dot products of up to 8 terms, identical combinations of neighbouring constraints are evaluated once, and independent operations
 * run side by side, level by level (csrc/wplan_wide.hpp).  For systems with WIDE rows (Poseidon: 63-term rows with general coefficients); a
 * chain of short rows (MiMC) has nothing to spread and is faster on the tape plan, which stays the default.
 * ZK_ERR_ARG: lanes not one of 4, 8, 16, 32, 64; a system whose temporaries do not fit the group's share of LDS (32 x lanes values) -- the
 * message names the level and the slots it needs.  zk_wplan_solve and zk_wplan_free take either kind of plan.
 *   zk_wplan_info   kind 0: tape (records_or_passes = records, products), kind 1: wide (passes, dataflow levels, operations = dots + steps +
 *                   hint operations, the widest level, the peak of LDS slots in use); products = field products of the constraint
 *                   evaluation per witness (coefficient products, a x b, the division by the target's coefficient), after deduplication */
typedef struct { uint32_t kind, lanes, records_or_passes, levels, ops, dots, steps, max_level_ops, lds_slots, products; } zk_wplan_stats;
int zk_wplan_create_wide(const zk_csr *A, const zk_csr *B, const zk_csr *C, uint32_t nC, uint32_t V, const uint8_t *known,
                         const zk_whint *hints, uint32_t n_hints, uint32_t lanes, int device, zk_wplan **out);
int zk_wplan_info(const zk_wplan *plan, zk_wplan_stats *out);
int zk_wplan_solve(zk_wplan *plan, void *d_w, uint32_t k, uint32_t *violations);
void zk_wplan_free(zk_wplan *plan);
/* TEST INFRASTRUCTURE, nothing on the proving path calls it: the program of a WIDE plan copied back from device memory, as 32-bit words --
 * the pass records in the layout at the top of csrc/wplan_wide.hpp ([pass][word of the record][lane in group], (passes + 1) x 19 x lanes words:
 * the program ends in one empty pass), then the coefficient table that the records index, 8 words per entry (Montgomery).  *n_words receives
 * the number of words whenever the plan is a wide one.  ZK_ERR_ARG for a tape plan and for cap < *n_words (nothing is copied). */
int zk_wplan_probe_program(const zk_wplan *plan, uint32_t *words, size_t cap, size_t *n_words);
int zk_dev_alloc(size_t bytes, int device, void **out);
int zk_dev_free(void *p);
int zk_dev_upload(void *dst, const void *src, size_t bytes);
int zk_dev_download(void *dst, const void *src, size_t bytes);

/* ---- MiMC Merkle tree in device memory (csrc/merkle.hpp, merkle.cpp): the tree of ethsnarks/merkletree.py, width 2, MerkleHasher_MiMC.
 * depth D = 1 .. 29, capacity 2^D leaves; level 0 holds the leaves, node j of level d + 1 = mimc_hash([n(d, 2j), n(d, 2j+1)], IV[d]); with n
 * leaves level d stores ceil(n / 2^d) nodes and a node that does not exist reads as unique(d, index) = sha256(be16(d) || be240(index)) mod r
 * (merkletree.py:24-34).  Nodes stay in Montgomery form in device memory; storage grows geometrically per level (reserve_leaves is a hint).
 * Codes: ZK_ERR_ARG for a null handle or argument, depth outside 1 .. 29, more leaves than the capacity, an index >= the size, a leaf >= r
 * (host leaves are checked before any device work, resident leaves by the kernel that takes them in), the root of an empty tree, a layout
 * that leaves the row; ZK_ERR_NOMEM when device memory runs out.  A call that fails with one of these leaves the tree as it was.
 * A zk_mtree is single-threaded like a zk_ctx.  Its work runs on a stream of its own and is complete when a call returns.
 *   zk_mtree_append            n leaves (n x 4 u64; Montgomery unless canonical != 0) become leaves size .. size + n - 1
 *   zk_mtree_append_resident   the same from device memory (the buffer is only read)
 *   zk_mtree_update            leaves[i] replaces leaf indices[i] and the ancestors are hashed again; an index that occurs more than
 *                              once takes the value of its LAST occurrence
 *   zk_mtree_root              canonical root; ZK_ERR_ARG for an empty tree (the reference's root is None then)
 *   zk_mtree_node              the reference's tree.leaf(level, offset): any node, level 0 .. D, offset < 2^(D - level), placeholders included
 *   zk_mtree_paths             for each of k indices the leaf and the D siblings (level 0 first), canonical; the address bits of index i
 *                              are (i >> d) & 1.  Either output may be NULL
 *   zk_mtree_fill_witnesses    for each of k indices writes into row j of a device witness buffer (row_elems Fr elements apart, Montgomery):
 *                              ONE at variable 0, the root, D address bits, D path elements, the leaf and n_iv (<= 29) level IVs at the
 *                              variable indices of the layout -- and nothing else of the row.  What zk_wplan_solve completes and
 *                              zk_prove_batch_submit_resident proves.  merkle_path_authenticator's allocation order (root, address bits,
 *                              path, leaf, IVs) is the layout {1, 2, 2 + D, 2 + 2 D, 3 + 2 D, 29}
 *   zk_mtree_fill_full_witnesses   the COMPLETE witness of the membership circuit for each of k indices: what zk_mtree_fill_witnesses writes, and
 *                              for every level d the level's variables in the gadgets' allocation order at level_var0 + d level_stride: the six of
 *                              merkle_path_selector (left_a, left_b, left, right_a, right_b, right), then
 *                                MiMC      outputs[0], outputs[1], 91 x (a, b, c, d) of cipher 0, 91 x (a, b, c, d) of cipher 1: 736 variables
 *                                Poseidon  105 x (x2, x4, x5) of the S-boxes in round order, the output: 322 variables
 *                              One lane per (row, level) computes them from the nodes the tree holds, so nothing is left for zk_wplan_solve:
 *                              variables 0 .. level_var0 + D level_stride - 1 of the allocation order (MiMC: level_var0 = 3 + 2 D + 29, Poseidon:
 *                              3 + 2 D) are all written, canonical Montgomery, byte-identical to what zk_wplan_solve leaves; nothing else of the
 *                              buffer is.  ZK_ERR_ARG, before any device work: node width 3 or 4, an empty tree, an index >= the size,
 *                              level_stride below 736 / 322, level blocks that leave the row or overlap an input variable of the layout,
 *                              n_iv != 0 (Poseidon) or n_iv < D (MiMC: the IVs are read).  k = 0 does nothing
 *   zk_mtree_update_seq        ORDERED updates with root-to-root transition witnesses: leaves[j] replaces leaf indices[j] for j = 0 .. k - 1 IN THE
 *                              GIVEN ORDER; an index may occur any number of times and every occurrence sees its predecessors.  The tree ends up node
 *                              for node as after k single zk_mtree_update calls.  roots_canon (may be NULL) receives k + 1 roots: [0] the root
 *                              before, [j + 1] the root after update j.  d_w != NULL: row j of the device witness buffer receives the COMPLETE
 *                              witness of the update circuit (gadgets.merkle_update_circuit: two markle_path_compute over the same address bits
 *                              and path, closed by result = old_root and result = new_root) for update j against the tree left by updates
 *                              0 .. j - 1: ONE, the inputs at the variable indices of the zk_mtree_update_layout, the OLD chain's level d at
 *                              level_var0 + d level_stride and the NEW chain's at level_var0 + (D + d) level_stride, each block as in
 *                              zk_mtree_fill_full_witnesses.  In the allocation order (old_root, new_root, D address bits, D path elements,
 *                              old_leaf, new_leaf, MiMC: 29 IVs; layout {1, 2, 3, 3 + D, 3 + 2 D, 4 + 2 D, 5 + 2 D, 29} or {.., 0, 0}, level_var0 =
 *                              5 + 2 D + n_iv) all variables 0 .. level_var0 + 2 D level_stride - 1 are written, canonical Montgomery,
 *                              byte-identical to what zk_wplan_solve leaves from the inputs alone; nothing else of the buffer is.  d_w == NULL:
 *                              the updates and the roots only.  The k chains advance together, one level per step, so the call costs D
 *                              dependent hashes whatever k (csrc/merkle.hpp).  ZK_ERR_ARG, before any device work: node width 3 or 4, an empty
 *                              tree, an index >= the size, a leaf >= r, and with d_w: level_stride below 736 / 322, level blocks that leave the
 *                              row or overlap an input variable, n_iv != 0 (Poseidon) or n_iv < D (MiMC); ZK_ERR_NOMEM for scratch that does not
 *                              fit.  Either code leaves the tree exactly as it was (only the last step of the call writes nodes).  k = 0 returns
 *                              roots_canon[0] and does nothing else.  (Added WITHOUT an ABI bump: detected by its symbol.)  MEASUREMENT ONLY:
 *                              ZK_MTREE_USEQ_TIMING=1 in the environment makes a call print the time of its host predecessor pass on stderr
 *   zk_mimc_constants          host-only: the 91 round constants and 29 level IVs the kernels use, canonical (either may be NULL)
 *   zk_mimc_hash2              out[i] = mimc_hash([left[i], right[i]], iv[i]) on the device, canonical in and out; an operand >= r is ZK_ERR_ARG
 *
 * ---- the same tree over Poseidon (csrc/poseidon.hpp): MerkleHasher_Poseidon of merkletree.py over the reference's DefaultParams = Poseidon128
 * (Fr, t = 6, 8 full + 57 partial rounds, x^5, constants from blake2b chains; ethsnarks/poseidon/permutation.py, src/gadgets/poseidon.hpp).
 *   zk_mtree_create_ex         hasher ZK_MTREE_HASH_MIMC (width 2 only) or ZK_MTREE_HASH_POSEIDON (node width 2, 3 or 4, width^depth <= 2^29:
 *                              depth <= 29, 18, 14); anything else is ZK_ERR_ARG.  zk_mtree_create(d, ..) = zk_mtree_create_ex(d, 2, MIMC, ..).
 *                              Poseidon: node j of level d + 1 = poseidon([n(d, w j), .., n(d, w j + w - 1)]) (no IV, the depth does not enter);
 *                              level d stores ceil(n / w^d) nodes, an absent node reads as unique(d, index) as above.  Every call above works
 *                              for every width with the same codes, capacity width^depth, offsets < width^(depth - level)
 *   zk_mtree_info              depth, width and hasher of a tree (any of the three may be NULL)
 *   zk_mtree_paths             at width w: w - 1 siblings per level, the other children of the own parent in node order (paths_canon holds
 *                              k x depth x (w - 1) elements); the address digit of index i on level d is (i / w^d) % w
 *   zk_mtree_fill_witnesses    Poseidon at width 2: layout.n_iv must be 0 (ZK_ERR_ARG otherwise: the circuit has no IV variables); the inputs of poseidon_membership_circuit, layout {1, 2, 2 + D, 2 + 2 D, 0, 0};
 *                              ZK_ERR_ARG at widths 3 and 4 (the reference has no wide path selector to build a circuit from)
 *   zk_poseidon_constants      host-only: the 65 round constants and the 6 x 6 matrix (row major), canonical (either may be NULL)
 *   zk_poseidon_hash           out[i] = poseidon(inputs[i n_in .. i n_in + n_in - 1]) on the device: state = the inputs, then zeros; the result is
 *                              state[0].  Canonical in and out; an operand >= r, n_in = 0 or n_in > 5 is ZK_ERR_ARG
 *   zk_poseidon_permute        the "chained" form: n full states of six elements through the permutation, in place, canonical
 * TEST / MEASUREMENT ONLY: ZK_POSEIDON_MIX=lmul | dot6 in the environment makes zk_poseidon_hash and zk_poseidon_permute run the kernel whose
 * MIX layer is six plain products per row, or the six-term dot product Field::ldot6 (the default, what the tree always uses).  Both give the
 * same values; the variable exists so that the two forms can be tested and timed against each other in one build. */
#define ZK_MTREE_HASH_MIMC 0
#define ZK_MTREE_HASH_POSEIDON 1
typedef struct zk_mtree zk_mtree;
typedef struct { uint32_t root_var, addr_var0, path_var0, leaf_var, iv_var0, n_iv; } zk_mtree_layout;
int zk_mtree_create(uint32_t depth, uint64_t reserve_leaves, int device, zk_mtree **out);
int zk_mtree_create_ex(uint32_t depth, uint32_t width, int hasher, uint64_t reserve_leaves, int device, zk_mtree **out);
int zk_mtree_info(const zk_mtree *t, uint32_t *depth, uint32_t *width, int *hasher);
void zk_mtree_free(zk_mtree *t);
int zk_mtree_size(const zk_mtree *t, uint64_t *n_leaves);
int zk_mtree_append(zk_mtree *t, const uint64_t *leaves, uint64_t n, int canonical);
int zk_mtree_append_resident(zk_mtree *t, const void *d_leaves, uint64_t n, int canonical);
int zk_mtree_update(zk_mtree *t, const uint64_t *indices, const uint64_t *leaves, uint32_t k, int canonical);
int zk_mtree_root(const zk_mtree *t, uint64_t root_canon[4]);
int zk_mtree_node(const zk_mtree *t, uint32_t level, uint64_t offset, uint64_t out_canon[4]);
int zk_mtree_paths(const zk_mtree *t, const uint64_t *indices, uint32_t k, uint64_t *leaves_canon /* k x 4 */, uint64_t *paths_canon /* k x depth x (width - 1) x 4 */);
int zk_mtree_fill_witnesses(const zk_mtree *t, const uint64_t *indices, uint32_t k, void *d_w, uint64_t row_elems, const zk_mtree_layout *layout);
int zk_mtree_fill_full_witnesses(const zk_mtree *t, const uint64_t *indices, uint32_t k, void *d_w, uint64_t row_elems,
                                 const zk_mtree_layout *layout, uint32_t level_var0, uint32_t level_stride);
typedef struct { uint32_t old_root_var, new_root_var, addr_var0, path_var0, old_leaf_var, new_leaf_var, iv_var0, n_iv; } zk_mtree_update_layout;
int zk_mtree_update_seq(zk_mtree *t, const uint64_t *indices, const uint64_t *leaves, uint32_t k, int canonical,
                        void *d_w, uint64_t row_elems, const zk_mtree_update_layout *layout,
                        uint32_t level_var0, uint32_t level_stride, uint64_t *roots_canon /* (k + 1) x 4, may be NULL */);
int zk_mimc_constants(uint64_t *round_constants_canon /* 91 x 4 */, uint64_t *ivs_canon /* 29 x 4 */);
int zk_mimc_hash2(const uint64_t *left, const uint64_t *right, const uint64_t *iv, uint32_t n, int device, uint64_t *out);
int zk_poseidon_constants(uint64_t *C_canon /* 65 x 4 */, uint64_t *M_canon /* 36 x 4, row major */);
int zk_poseidon_hash(const uint64_t *inputs /* n x n_in x 4 */, uint32_t n_in, uint32_t n, int device, uint64_t *out /* n x 4 */);
int zk_poseidon_permute(uint64_t *states /* n x 6 x 4, in place */, uint32_t n, int device);

/* ---- Baby JubJub (csrc/jubjub.hpp, jubjub.cpp): the native side of ethsnarks/jubjub.py, pedersen.py and eddsa.py.  The curve is
 * a x^2 + y^2 = 1 + d x^2 y^2 over Fr, a = 168700, d = 168696, order 8 L.  Every field value is canonical (4 x u64 limbs, below r), a point is x
 * then y (8 limbs); the identity is (0, 1).  Device calls take n items and run ONE kernel launch each, whatever n is.
 * Codes: ZK_ERR_ARG -- and NOTHING is written -- for a null argument, a coordinate, s or MiMC message element >= r, a window > 7 (among the count
 * windows of its row), a window count of 0, above the stride or above the hasher's capacity, a name longer than 28 bytes, a base point index
 * above 0xFFFF, an unknown operation or scheme, msg_len outside 1 .. 4096, max_windows outside 1 .. 15872.
 * OFF-CURVE POINTS, the one deliberate difference from the reference (which never checks, and whose affine formulas then divide by zero or return
 * garbage): zk_jj_point_op, zk_jj_scalar_mul and the B of zk_eddsa_create answer ZK_ERR_ARG (and write nothing); zk_eddsa_verify_batch gives
 * verdict 0 to a signature whose A or R is not on the curve.  Everything ON the curve behaves as the reference: the addition is complete, so the
 * identity, P + P, P + (-P) and the eight low-order points need no special case; s is not required to be below L (s + L verifies when s does);
 * low-order A and R are accepted and evaluated.
 *   zk_jj_hash_to_point        host-only: Point.from_hash -- y = sha256(data) mod r, incremented until x exists; x the root with x > r - x; times 8
 *   zk_jj_pedersen_basepoint   host-only: from_hash("%-28s%04X" % (name, i)); name is NUL-terminated, at most 28 bytes
 *   zk_jj_point_op             out[i] = p[i] + q[i] (ZK_JJ_OP_ADD: the unified addition, also when p[i] == q[i]), 2 p[i] (ZK_JJ_OP_DOUBLE: the
 *                              dedicated doubling) or -p[i] (ZK_JJ_OP_NEGATE); q is read by ZK_JJ_OP_ADD only
 *   zk_jj_scalar_mul           out[i] = scalars[i] points[i]; a scalar is ANY 256-bit integer (4 limbs; 0, >= L, >= 8 L, 2^256 - 1 are all defined)
 *   zk_pedersen_create         the hasher of pedersen_hash_windows(name, ..) for up to max_windows windows: the multiples (1 .. 4) 16^j B_s of every
 *                              window position go to device memory once
 *   zk_pedersen_hash           n hashes; row i of windows (stride bytes apart, each 0 .. 7) holds counts[i] windows (counts == NULL: stride each).
 *                              Window w adds ((w & 3) + 1) 16^(j % 62) B_(j / 62), negated when w > 3; a padding window is NOT neutral
 *   zk_pedersen_table          host-only: the 4 table points of each of n_windows window positions from first_window on (n_windows x 4 x 8 limbs)
 *   zk_eddsa_create            a verifier for one scheme: ZK_EDDSA_MIMC (MiMCEdDSA: t = mimc_hash([R.x, R.y, A.x, A.y, m..], 0) with the constants of
 *                              seed "EdDSA_Verify.RAM"; msg_len = field elements per message), ZK_EDDSA_PURE (PureEdDSA: t = the x of
 *                              pedersen_hash_bits("EdDSA_Verify.RAM", bits(R.x) || bits(A.x) || M); msg_len = bytes per message) or ZK_EDDSA_HASH
 *                              (EdDSA: as pure with M = the x of pedersen_hash_bytes("EdDSA_Verify.M", msg)).  B == NULL: the generator
 *   zk_eddsa_verify_batch      verdicts[i] = (s[i] B == R[i] + t A[i]); A, R: n x 8, s: n x 4, msgs: n x msg_len bytes (n x msg_len x 4 limbs for
 *                              ZK_EDDSA_MIMC).  t is computed on the device
 *   zk_eddsa_fill_witnesses    (ZK_EDDSA_MIMC only) for each of n signatures the COMPLETE witness row of the MiMC-EdDSA circuit -- eddsa_mimc_circuit of
 *                              ethsnarks_amd/jubjub_gadgets.py: PointValidator(R), fixed_base_mul(B, the 254 bits of s), the MiMC hash, field2bits_strict
 *                              and a range check of the bits of t, ScalarMult(A, bits of t), PointAdder(R, t A), lhs == rhs -- into row i of a device
 *                              buffer (row_elems Fr elements apart), canonical Montgomery: what zk_wplan_solve leaves and
 *                              zk_prove_batch_submit_resident reads, every element equal to the front end's generate_r1cs_witness.  The front
 *                              end defines the row: zk_eddsa_layout names the variable index of the first element of every segment (and the
 *                              stride of the 253 doubler / conditional / adder steps), n_vars + 1 elements in all; the kernel computes no offset
 *                              of its own.  verdicts[i] is what zk_eddsa_verify_batch answers for the item.  A WELL-FORMED WRONG signature gets
 *                              its full row and verdict 0: only the two closing equalities fail.  A MALFORMED item -- A or R off the curve, or
 *                              s >= 2^254 (s is ANY 256-bit integer here, not required to be below r) -- gets verdict 0 and its row is NOT
 *                              TOUCHED.  An R of low order gets its row and the verifier's verdict, but the circuit's PointValidator rejects it.
 *                              ZK_ERR_ARG and nothing written: another scheme, layout.msg_len != the verifier's, n_vars + 1 > row_elems, a
 *                              segment outside variables 1 .. n_vars or overlapping another, a coordinate or message element >= r.
 *                              One lane per signature walks the three point chains (253 doublings of A, 253 + 126 additions) projectively and
 *                              pays ONE field inversion per witness, whatever the number of bits (csrc/jubjub.hpp)
 * A zk_pedersen and a zk_eddsa are single-threaded like a zk_ctx; their work runs on a stream of their own and is complete when a call returns. */
#define ZK_JJ_OP_ADD 0
#define ZK_JJ_OP_DOUBLE 1
#define ZK_JJ_OP_NEGATE 2
#define ZK_EDDSA_MIMC 0
#define ZK_EDDSA_PURE 1
#define ZK_EDDSA_HASH 2
typedef struct zk_pedersen zk_pedersen;
typedef struct zk_eddsa zk_eddsa;
int zk_jj_hash_to_point(const uint8_t *data, size_t len, uint64_t out[8]);
int zk_jj_pedersen_basepoint(const char *name, uint32_t i, uint64_t out[8]);
int zk_jj_point_op(int op, const uint64_t *p /* n x 8 */, const uint64_t *q /* n x 8 */, uint32_t n, int device, uint64_t *out /* n x 8 */);
int zk_jj_scalar_mul(const uint64_t *points /* n x 8 */, const uint64_t *scalars /* n x 4 */, uint32_t n, int device, uint64_t *out /* n x 8 */);
int zk_pedersen_create(const char *name, uint32_t max_windows, int device, zk_pedersen **out);
void zk_pedersen_free(zk_pedersen *h);
int zk_pedersen_hash(zk_pedersen *h, const uint8_t *windows /* n x stride */, const uint32_t *counts /* n, or NULL */, uint32_t stride, uint32_t n, uint64_t *out /* n x 8 */);
int zk_pedersen_table(const zk_pedersen *h, uint32_t first_window, uint32_t n_windows, uint64_t *out /* n_windows x 4 x 8 */);
int zk_eddsa_create(int scheme, const uint64_t *B /* 8 limbs, or NULL */, uint32_t msg_len, int device, zk_eddsa **out);
void zk_eddsa_free(zk_eddsa *v);
int zk_eddsa_verify_batch(zk_eddsa *v, const uint64_t *A, const uint64_t *R, const uint64_t *s, const void *msgs, uint32_t n, uint8_t *verdicts /* n */);
/* first variable of each segment of a witness row (variable 0 is ONE): A.x, A.y | msg_len message elements | R.x, R.y | 254 bits of s | the zero IV |
 * validator: 3 x 6 doubler variables, Y, M, xx, yy | 127 x (x, y) window lookups | 126 x 7 fixed-base adder variables | 4 + msg_len hash outputs, then
 * (4 + msg_len) x 91 x (a, b, c, d) | 254 bits of t, 253 results, 254 comparisons | 99 range-check products | conditionals[0] (2) | per step
 * i = 1 .. 253 at + (i - 1) step_stride: 6 doubler, 2 conditional, 7 adder variables | the 7 variables of the last adder */
typedef struct {
    uint32_t msg_len, n_vars, ax_var, msg_var0, rx_var, s_bit0, iv_var, validator_var0, window_var0, fixed_adder_var0, mimc_var0, t_bit0,
             t_range_var0, cond0_var, doubler_var0, cond_var0, adder_var0, step_stride, last_adder_var0;
} zk_eddsa_layout;
int zk_eddsa_fill_witnesses(zk_eddsa *v, const uint64_t *A /* n x 8 */, const uint64_t *R /* n x 8 */, const uint64_t *s /* n x 4 */, const uint64_t *msgs /* n x msg_len x 4 */,
                            uint32_t n, void *d_w, uint64_t row_elems, const zk_eddsa_layout *layout, uint8_t *verdicts /* n */);
/* zk_eddsa_fill_witnesses with `lanes` lanes per witness -- the same contract, the same refusals with nothing written, the same rows byte for byte.
 * lanes = 1 IS zk_eddsa_fill_witnesses.  lanes = 2 or 4 shortens the dependent chain of one witness (14 816 field products on one lane) to about
 * 10 700 or 9 300: the lanes are one lane of each wave of a workgroup of 64 x lanes threads, they split the two forward walks, the way back after
 * the one inversion and the gadgets' products, and meet at two barriers (csrc/jubjub.hpp k_eddsa_fill_wide).  For small batches, where
 * the call's time is that chain's latency; the total work is not smaller.  Any other value of lanes: ZK_ERR_ARG.  The library never chooses lanes itself. */
int zk_eddsa_fill_witnesses_wide(zk_eddsa *v, const uint64_t *A /* n x 8 */, const uint64_t *R /* n x 8 */, const uint64_t *s /* n x 4 */, const uint64_t *msgs /* n x msg_len x 4 */,
                                 uint32_t n, void *d_w, uint64_t row_elems, const zk_eddsa_layout *layout, uint8_t *verdicts /* n */, uint32_t lanes);
/* The PureEdDSA circuit (ZK_EDDSA_PURE only) -- eddsa_pure_circuit of ethsnarks_amd/jubjub_gadgets.py, the reference's PureEdDSA gadget: PointValidator(R),
 * fixed_base_mul(B, the 254 bits of s), field2bits_strict of R.x and of A.x, the windowed Pedersen hash "EdDSA_Verify.RAM" of those bits and the
 * message bits IN THE CIRCUIT (fixed_base_mul_zcash: lookup_signed_3bit, MontgomeryAdder, MontgomeryToEdwards, PointAdder), field2bits_strict of its
 * x, a range check behind each of the three decompositions, ScalarMult(A, bits of t), PointAdder(R, t A), lhs == rhs.  With W = ceil((508 + 8 msg_len) / 3)
 * windows and S = ceil(W / 62) segments, first variable of each segment of a row: A.x, A.y | 8 msg_len message bits (a byte's most significant first) |
 * R.x, R.y | 254 bits of s | 3 W - 508 - 8 msg_len zero padding bits | validator (22) | 127 x (x, y) | 126 x 7 | R.x: 254 bits, 253 results, 254
 * comparisons | 99 range products | A.x likewise | W x (b0b1, Montgomery y) | (W - S) x (lambda, X3, Y3) | S x (x, y) of the converters, the lone last
 * window's first | (S - 1) x 7 Edwards adder variables | t likewise | conditionals[0] (2) | per step doubler (6), conditional (2), adder (7), step_stride
 * apart | the last adder (7).
 * zk_eddsa_fill_pure_witnesses is zk_eddsa_fill_witnesses for this circuit, with the same contract: the front end defines every offset; ZK_ERR_ARG and
 * nothing written for a handle that is not ZK_EDDSA_PURE, row_elems < n_vars + 1, a layout whose msg_len is not the verifier's, a segment outside
 * variables 1 .. n_vars or overlapping another, a coordinate >= r; a well-formed wrong signature gets its full row and verdict 0; a malformed item
 * (A or R off the curve, s >= 2^254) gets verdict 0 and an untouched row; verdicts[i] is zk_eddsa_verify_batch's.  One kernel launch, one lane per
 * signature, TWO field inversions per witness whatever the number of windows (csrc/jubjub.hpp k_eddsa_fill_pure). */
typedef struct {
    uint32_t msg_len, n_vars, ax_var, msg_bit0, rx_var, s_bit0, pad_bit0, validator_var0, window_var0, fixed_adder_var0, rx_bit0, rx_range_var0,
             ax_bit0, ax_range_var0, hash_window_var0, mont_adder_var0, converter_var0, edwards_adder_var0, t_bit0, t_range_var0, cond0_var,
             doubler_var0, cond_var0, adder_var0, step_stride, last_adder_var0;
} zk_eddsa_pure_layout;
int zk_eddsa_fill_pure_witnesses(zk_eddsa *v, const uint64_t *A /* n x 8 */, const uint64_t *R /* n x 8 */, const uint64_t *s /* n x 4 */, const uint8_t *msgs /* n x msg_len bytes */,
                                 uint32_t n, void *d_w, uint64_t row_elems, const zk_eddsa_pure_layout *layout, uint8_t *verdicts /* n */);
/* The EdDSA circuit of the "hash" scheme (ZK_EDDSA_HASH only) -- EddsaHashCircuit of ethsnarks_amd/jubjub_gadgets.py, the reference's EdDSA gadget: the
 * PureEdDSA circuit above over the 254 strict bits of M.x, M = the windowed Pedersen hash "EdDSA_Verify.M" of the message bits, hashed IN THE CIRCUIT too,
 * with a range check behind that fourth decomposition.  The hash "EdDSA_Verify.RAM" covers 3 x 254 bits: W = 254 windows, S = 5 segments (62, 62, 62,
 * 62, 6), no padding bit, no lone window.  The message hash has W_m = ceil(8 msg_len / 3) windows in S_m = ceil(W_m / 62) segments, a lone last window
 * when W_m % 62 == 1.  zk_eddsa_hash_layout: every member of zk_eddsa_pure_layout but pad_bit0, with the same meaning, then the message hash's:
 * m_pad_bit0 ((-8 msg_len) mod 3 zero padding bits) | m_window_var0 (W_m x (b0b1, Montgomery y)) | m_mont_adder_var0 ((W_m - S_m) x 3) |
 * m_converter_var0 (S_m x (x, y), the lone window's first) | m_edwards_adder_var0 ((S_m - 1) x 7) | m_bit0 (254 bits, 253 results, 254 comparisons of
 * M.x) | m_range_var0 (99 range products).  A segment WITHOUT elements (no padding bit when msg_len is a multiple of 3; no Edwards adder when
 * msg_len <= 23) is not there: its member is not looked at.
 * zk_eddsa_fill_hash_witnesses has the contract of zk_eddsa_fill_pure_witnesses: ZK_ERR_ARG and nothing written for a handle that is not ZK_EDDSA_HASH,
 * row_elems < n_vars + 1, a layout whose msg_len is not the verifier's, a segment outside variables 1 .. n_vars or overlapping another, a coordinate
 * >= r, a null argument with n > 0; n = 0 succeeds; a well-formed wrong signature gets its full row and verdict 0; a malformed item (A or R off the
 * curve, s >= 2^254) gets verdict 0 and an untouched row; verdicts[i] is zk_eddsa_verify_batch's.  One kernel launch, one lane per signature, THREE
 * field inversions per witness whatever msg_len (csrc/jubjub.hpp k_eddsa_fill_hash).  The handle's first call builds the tables that only the
 * fill reads -- the circuit's fixed-base windows of B and the Montgomery form of both Pedersen tables, 32 x (1 524 + 8 (254 + W_m)) bytes of device
 * memory, freed with the handle -- so zk_eddsa_create costs a verify-only user what it did; like every call on a zk_eddsa it must not run beside
 * another call on the same handle. */
typedef struct {
    uint32_t msg_len, n_vars, ax_var, msg_bit0, rx_var, s_bit0, validator_var0, window_var0, fixed_adder_var0, rx_bit0, rx_range_var0,
             ax_bit0, ax_range_var0, hash_window_var0, mont_adder_var0, converter_var0, edwards_adder_var0, t_bit0, t_range_var0, cond0_var,
             doubler_var0, cond_var0, adder_var0, step_stride, last_adder_var0, m_pad_bit0, m_window_var0, m_mont_adder_var0, m_converter_var0,
             m_edwards_adder_var0, m_bit0, m_range_var0;
} zk_eddsa_hash_layout;
int zk_eddsa_fill_hash_witnesses(zk_eddsa *v, const uint64_t *A /* n x 8 */, const uint64_t *R /* n x 8 */, const uint64_t *s /* n x 4 */, const uint8_t *msgs /* n x msg_len bytes */,
                                 uint32_t n, void *d_w, uint64_t row_elems, const zk_eddsa_hash_layout *layout, uint8_t *verdicts /* n */);
/* The signer (csrc/eddsa_sign.hpp): _SignatureScheme.sign of ethsnarks/eddsa.py for n keys and messages in ONE kernel launch, one lane per
 * signature.  Scheme, B and msg_len are the handle's; msgs as zk_eddsa_verify_batch takes them.  Per item: r = int_le(SHA-512(key as 32 little-endian
 * bytes || the bytes of M)) mod L, R = r B, A = key B, t = H(R, A, M) as the verifier computes it, s = (r + key t) mod 8 L.  The bytes of M: the message
 * elements as 32 little-endian bytes each (ZK_EDDSA_MIMC), the message bytes (ZK_EDDSA_PURE), the point pedersen_hash_bytes("EdDSA_Verify.M", msg) as x
 * then y, 32 little-endian bytes each (ZK_EDDSA_HASH).  The handle's first call builds a fixed-base table of B (98 304 bytes of device memory, freed
 * with the handle).  ZK_ERR_ARG for the WHOLE call, and nothing written: a null argument, a key that is 0 or >= L (the reference raises "Strict parsing
 * of k failed"), a ZK_EDDSA_MIMC message element >= r.  n = 0 succeeds and writes nothing.
 * WHERE THE SECRETS GO.  The keys are copied to a device buffer and each lane writes its nonce to a buffer beside it; both are zeroed before the call
 * returns, on every path.  The kernel reads every digit of key and nonce from those buffers at the point of use and keeps neither scalar in a private
 * array nor in a register across a call, so that no copy of them is left in the lanes' scratch memory, which nobody clears (checked in the gfx950
 * assembly; what a call may still save there is the table address chosen by ONE digit).  The library itself makes no host copy of the keys, but it
 * uploads them from the caller's pageable memory, which the HIP runtime stages through a pinned buffer of its own that is not wiped; a caller who
 * minds passes page-locked memory (zk_host_alloc) and zeroes it.  The first call on a handle builds the table: like every call on a zk_eddsa it must
 * not run beside another call on the same handle (the single-thread rule above).
 *   1. NOT CONSTANT TIME.  The table entries a lane reads are chosen by the digits of the key and of the nonce, and the reductions end in
 *      data-dependent subtractions.  The signer is for bulk generation of signatures, not for keys that must withstand a co-tenant of the device.
 *   2. s IS THE INTEGER mod 8 L, and 8 L lies slightly above the field modulus r.  A value in [r, 8 L) has a probability below 2^-160; the reference's
 *      Signature would reduce such a value mod r and break the signature; zk_eddsa_verify_batch answers ZK_ERR_ARG for it.
 * zk_eddsa_sign_probe is for tests only: the SAME device functions the signer uses, one lane per item.  op 0: SHA-512 of n messages of len bytes
 * each (a: n x len bytes) -> n x 64 bytes; op 1: n 512-bit little-endian integers (a: n x 8 limbs) mod L -> n x 4 limbs; op 2: (a + b c) mod 8 L
 * for any 256-bit a, b, c (n x 4 limbs each) -> n x 4 limbs.  ZK_ERR_ARG: an unknown op, a null argument, n above 2^20 or more than 2^30 input bytes. */
int zk_eddsa_sign_batch(zk_eddsa *v, const uint64_t *keys /* n x 4 */, const void *msgs /* as zk_eddsa_verify_batch */, uint32_t n,
                        uint64_t *A /* n x 8 */, uint64_t *R /* n x 8 */, uint64_t *s /* n x 4 */);
int zk_eddsa_sign_probe(int op, const void *a, const void *b, const void *c, uint32_t n, uint32_t len, int device, void *out);

/* ---- measurement aids (bench.py): kernel launches issued by this library so far; between zk_profile_begin() and
 * zk_profile_end() every launch is bracketed by a HIP event pair on its own stream -- the sum of the kernel durations
 * (overlapping kernels counted each), their number, and "name calls ms" lines per kernel come back */
uint64_t zk_launch_count(void);
int zk_profile_begin(void);
int zk_profile_end(float *kernel_ms_sum, uint32_t *launches, char *buf, size_t cap);
int zk_device_info(int device, uint32_t *compute_units, uint32_t *clock_mhz, char *name, size_t name_cap);
/* "domain:bus:device.function" of the HIP device (multi-GPU runs report it per rank: proof that the ranks sit on distinct GPUs) */
int zk_device_pci_bus_id(int device, char *buf, size_t cap);

/* ---- kernel-level entry points (parity tests / micro-benchmarks); host buffers in and out */
int zk_ntt(uint64_t *data, uint32_t logm, int inverse, int coset, int device);
int zk_witness_map(zk_ctx *ctx, const uint64_t *witness, int canonical, uint64_t *h_out /* (m+1) x 4 */);
int zk_msm_g1(const uint64_t *bases, const uint64_t *scalars, uint32_t n, uint32_t c, int device, uint64_t out_affine[8]);
int zk_msm_g2(const uint64_t *bases, const uint64_t *scalars, uint32_t n, uint32_t c, int device, uint64_t out_affine[16]);
/* host-only: n Fr elements between canonical and Montgomery form, in place (adapters whose field objects are opaque) */
int zk_fr_convert(uint64_t *io, uint32_t n, int to_montgomery);
int zk_field_mul(const uint64_t *a, const uint64_t *b, uint64_t *out, uint32_t n, int field /* 0 Fr, 1 Fq */, int device);
/* k independent products of n pairs (affine Montgomery, all-zero = infinity, points in the order-r groups; n k <= 2^24):
 * is_one[i] = 1 iff prod_j e(g1[i*n+j], g2[i*n+j]) = 1 */
int zk_pairing_check(const uint64_t *g1, const uint64_t *g2, uint32_t n, uint32_t k, int device, uint8_t *is_one);
/* host-only: one operation of the pairing's Fq12 tower (csrc/pairing.hpp) on canonical elements, 12 x 4 u64 in the order
 * c0.c0.c0, c0.c0.c1, c0.c1.c0, ... (coefficient a_ij of v^i w^j at index 6 j + 2 i + {0: real, 1: u part}).
 * op: 0 a b, 1 a^2, 2 1/a, 3..5 a^(q^1..3), 6 cyclotomic square, 7 a^((q^6-1)(q^2+1)), 8 final exponentiation, 9 conjugate (b unused but for 0) */
int zk_pairing_tower_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out);
/* ---- arithmetic probe: TEST INFRASTRUCTURE, nothing on the proving path calls it.  One primitive of csrc/bn254.hpp per launch, applied
 * to n <= 2^20 cases whose operands are taken AS GIVEN (raw 8 x u32 limb values, Montgomery where the primitive expects it; no range
 * check) and whose RAW result limbs come back: no canon, no fix-up.  On the device this is the hand-written gfx950 layer (fips_asm.hpp,
 * the loose domain [0, 2p)); in the CPU emulation the loose names are the strict host operations.
 *   op = ZK_PROBE_FR / _FQ / _FQ2 / _G1 / _G2 plus an index.  A "word" is one field element of 4 u64; an Fq2 element is 2 words
 *   (c0, c1), an affine point 2 elements (x, y), an XYZZ point 4 elements (X, Y, ZZ, ZZZ).
 *   ZK_PROBE_FR, ZK_PROBE_FQ (operands a, b, ... one word each; one result word unless noted):
 *      0 add(a, b)   1 sub(a, b)   2 neg(a)   3 mul(a, b)   4 reduce_once(a)   5 canon(a)
 *      6 lmul(a, b)  7 lsqr(a)     8 ladd(a, b)  9 lsub(a, b)  10 ldbl(a)  11 lneg(a)  12 lis_zero(a) (0 or 1 in the low limb)
 *     13 lneg_op(a)  14 lmul(a, lneg_op(b))
 *     15 lmul2(a, b, c, d)   16 lmul2(a, b, c, lneg_op(d))
 *     17 lmul4(a, .., h)     18 lmul4(a, b, c, lneg_op(d), e, f, g, lneg_op(h))
 *     19 lmul_x2(a, b, c, d) -> (a b, c d): 2 words      20 lmul2_x2(a, .., h) -> (a b + c d, e f + g h): 2 words
 *     21 to_mont(a)  22 from_mont(a)  23 inv(a)
 *     25 ldot6(a0 .. a5, b0 .. b5) = a0 b0 + .. + a5 b5 with one reduction: 12 operand words, a0 .. a5 then b0 .. b5 (the a loose, the b
 *        CANONICAL: the precondition of Field::ldot6), one result word.  (24 is not assigned and stays an unknown op: the probe's own
 *        argument test uses it as the first index past the table.)
 *     26 lsqr_pair(a, b) -> (a^2, b^2): 2 words (the dual squaring of the G1 mixed addition)
 *   ZK_PROBE_FQ2 (operands and result are Fq2 elements):
 *      0 lmul(a, b)  1 lsqr(a)  2 lmul2(a, b, c, d)  3 ladd(a, b)  4 lsub(a, b)  5 lis_zero(a) (0 or 1 in the low limb of c0)
 *      6 ldbl(a)  7 lneg(a)  8 canon(a)  9 inv(canon(a)) (strict result; 0 -> 0: the form pairing.hpp's f2inv uses)
 *     10 eq(canon(a), canon(b)) (0 or 1 in the low limb of c0)
 *   ZK_PROBE_G1, ZK_PROBE_G2 (Curve<Fq>, Curve<Fq2>; A = affine point, X = XYZZ point):
 *      0 dbl_affine(A) -> X   1 dbl(X) -> X   2 madd(X, A) -> X   3 madd_pairs(X, A) -> X   4 add(X, X) -> X
 *      5 dbl_q(X)   6 add_q(X, X)   7 madd_q(X, A): the case runs on four adjacent lanes that hold the same operands, the four
 *        lanes' results come back one after the other (4 X per case)
 *      8 canon(X) -> X   9 to_affine(X) -> A
 * zk_arith_probe_shape (host-only): words per case that `in` holds and `out` receives; ZK_ERR_ARG for an unknown op. */
#define ZK_PROBE_FR 0x000
#define ZK_PROBE_FQ 0x100
#define ZK_PROBE_FQ2 0x200
#define ZK_PROBE_G1 0x300
#define ZK_PROBE_G2 0x400
int zk_arith_probe_shape(int op, uint32_t *in_words, uint32_t *out_words);
int zk_arith_probe(int op, const uint64_t *in, uint32_t n, uint64_t *out, int device);
/* ---- pairing probe: TEST INFRASTRUCTURE, nothing on the verifying path calls it.  One function of csrc/pairing.hpp per launch, one lane
 * per case (blocks of 64), n <= 2^12 cases.  The kernels sit in csrc/verify_gpu.cpp and call the compiled bodies the batch verifier calls
 * (the tower functions are real, non-inlined device functions on operands in the lane's scratch memory).  Operands are taken AS GIVEN
 * (raw 8 x u32 limb values, Montgomery form, loose domain [0, 2q); no range check), RAW result limbs come back: no canon.  In the CPU
 * emulation the loose names are the strict host operations.  (zk_pairing_tower_op above stays the host-only, canonical form.)
 *   A "word" is one Fq element of 4 u64.  fe2 = 2 words (c0, c1), fe6 = 6 (c0, c1, c2), fe12 = 12 in the order of zk_pairing_tower_op;
 *   G1 = affine point, 2 words; G2 = affine twist point, 4 words (all-zero: infinity); T = G2Hom (X, Y, Z), 6 words; L = LineC (a, b, c),
 *   6 words; a flag or skip operand is one word whose low limb is 0 or 1; "~" marks the form whose output aliases its first operand.
 *      0 f6mul(a, b)   1 ~f6mul   2 f6mul01(a, b0, b1)   3 f6inv(a)   4 f6mulv(a)   5 f6add(a, b)   6 f6sub(a, b)   7 f6neg(a)
 *      8 f2mulxi(a)    9 f2muls(a, s: 1 word)   10 f2conj(a)
 *     11 f12mul(a, b) 12 ~f12mul  13 f12sqr(a)  14 ~f12sqr  15 f12inv(a)  16 ~f12inv  17 f12conj(a)  18 .. 20 f12frob<1 .. 3>(a)
 *     21 f12cycsqr(a) 22 ~f12cycsqr   23 f12mul034(f, c0, d0, d1) -> f   24 f12eq(a, b) -> flag   25 f12is_one(a) -> flag
 *     26 f12canon(a) (strict: every coefficient < q)   27 f12exp_negz(a)   28 final_exp_easy(a)   29 final_exp(a)
 *     30 dbl_step(T) -> (T', L)   31 add_step(T, Q: G2) -> (T', L)   32 g2_frob1(Q) -> G2   33 g2_negfrob2(Q) -> G2
 *     34 ell(f, L, P: G1, skip) -> f
 *     35 .. 37 miller_multi with nv = 1 .. 3 variable pairs, operands P_0 .. P_(nv-1) then Q_0 .. Q_(nv-1) -> f before the final exponentiation
 *     38, 39  the fixed-Q route with nf = 1, 2: operands P_0 .. then Q_0 .. then one word fskip (low limb: bit j skips pair j); the lane
 *             runs miller_precompute for its Q into global storage the host allocates, then miller_multi(nv = 0, nf, fskip) -> f
 *     40 .. 42 k_pair_product itself with n = 1 .. 3 pairs per case (operands as 35 .. 37), its `values` returned: FE(prod ML), canonical
 *     43 g2_on_curve(Q) -> flag   44 g2_in_subgroup(Q) -> flag   45 g1_on_curve(P) -> flag
 * zk_pairing_probe_shape (host-only): words per case that `in` holds and `out` receives; ZK_ERR_ARG for an unknown op.
 * zk_vctx_probe_prepare (TEST INFRASTRUCTURE as well): runs the prepare kernel of zk_verify_batch alone on a live context and returns the
 * k records it hands to the pairing kernel, 42 u64 each: A, -acc, -C (G1), B (G2) as raw Montgomery limbs, (0, 0) = infinity, then `ok`
 * in the low 32 bits of word 40 (1: coordinates < q, inputs < r, A and C on the curve) and padding.  Arguments as zk_verify_batch. */
int zk_pairing_probe_shape(int op, uint32_t *in_words, uint32_t *out_words);
int zk_pairing_probe(int op, const uint64_t *in, uint32_t n, uint64_t *out, int device);
int zk_vctx_probe_prepare(zk_vctx *v, const zk_proof *proofs, const uint64_t *inputs_canon, uint32_t k, uint64_t *out_points);

#ifdef __cplusplus
}
#endif
#endif
