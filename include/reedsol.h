/*
 * reedsol.h — C ABI of the MI355X-native Reed-Solomon engine (librs_amd.so).
 *
 * Drop-in for the encode/decode path of usebeforefree/reed-solomon-cc
 * (Zig, snapshot 2025-12-12): systematic RS over GF(2^16) in a Cantor basis,
 * Lin-Chung-Han additive FFT, "high rate" codec. Every entry point cites the
 * reference interface it replaces (paths relative to the reference repo).
 * Plain pointers and sizes only; no HIP or torch types in any signature
 * (a stream is passed as an opaque `void*`, i.e. a hipStream_t or NULL).
 *
 * Shard layout: the reference's own — a shard of shard_bytes is L =
 * shard_bytes/64 chunks of 64 B; in a chunk, bytes [0,32) are the low bytes
 * and [32,64) the high bytes of 32 GF(2^16) symbols (Generic.zig:152-156,
 * root.zig:373-383). No transposition anywhere.
 *
 * Every function returns an rs_status; none aborts. Results are bit-exact
 * with the reference algorithm (RS_FLAG_REF_LITERAL reproduces its two
 * arithmetic/schedule defects D1/D2).
 */
#ifndef REEDSOL_AMD_H
#define REEDSOL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes. 1..11 mirror the Zig error set of root.zig
 * (TooFewOriginalShards .. Overflow); 12.. are conditions where the
 * reference panics or that only a device engine can hit. */
typedef enum rs_status {
  RS_OK = 0,
  RS_ERR_TOO_FEW_ORIGINAL_SHARDS = 1,  /* root.zig:20, 139 */
  RS_ERR_NOT_ENOUGH_SHARDS = 2,        /* root.zig:58, 272 */
  RS_ERR_INVALID_SHARD_SIZE = 3,       /* root.zig:103, 201 */
  RS_ERR_UNSUPPORTED_SHARD_COUNT = 4,  /* root.zig:398, 407 */
  RS_ERR_TOO_MANY_ORIGINAL_SHARDS = 5, /* root.zig:129 */
  RS_ERR_DIFFERENT_SHARD_SIZE = 6,     /* root.zig:130, 243, 259 */
  RS_ERR_INVALID_SHARD_INDEX = 7,      /* root.zig:240, 254 */
  RS_ERR_DUPLICATE_SHARD_INDEX = 8,    /* root.zig:241, 256 */
  RS_ERR_TOO_MANY_SHARDS = 9,          /* root.zig:242, 258 */
  RS_ERR_OUT_OF_MEMORY = 10,           /* allocator failure */
  RS_ERR_OVERFLOW = 11,                /* std.math.ceilPowerOfTwo */
  RS_ERR_LOW_RATE_UNSUPPORTED = 12,    /* root.zig:120, 227 @panic("TODO"); no longer returned (every path serves low-rate codes) */
  RS_ERR_SHARD_TAIL_UNSUPPORTED = 13,  /* root.zig:385 @panic("TODO"); no longer returned (tails are coded) */
  RS_ERR_INVALID_ARGUMENT = 14,        /* NULL pointer / bad stride */
  RS_ERR_DEVICE = 15,                  /* HIP runtime error (message: rs_last_error()) */
  RS_ERR_NO_DEVICE = 16,               /* no gfx950 device visible */
} rs_status;

/* flags for the *_dev and engine entry points */
#define RS_FLAG_CORRECTED 0u
#define RS_FLAG_QUIRK_D1 1u /* Generic.zig:283: t1_hi used for nibble 0 of the hi product */
#define RS_FLAG_QUIRK_D2 2u /* root.zig:151: `<` drops the last full chunk when k % chunk == 0 */
#define RS_FLAG_REF_LITERAL (RS_FLAG_QUIRK_D1 | RS_FLAG_QUIRK_D2)

typedef void *rs_stream_t; /* hipStream_t, or NULL for the default stream */

/* ------------------------------------------------------------------ info */
const char *rs_version(void);
const char *rs_status_name(int status);  /* "NotEnoughShards", ... (Zig error names) */
const char *rs_last_error(void);         /* thread-local detail for the last non-OK status */
/* root.zig:397-415 useHighRate: 1 high rate, 0 low rate, negative = -rs_status */
int rs_use_high_rate(uint64_t original_count, uint64_t recovery_count);

/* ------------------------------------------- one-shot host API (root.zig:14-84)
 * Host buffers in, host buffers out; internally H2D -> fused HIP kernel -> D2H.
 * Generalises the reference's 64-byte-typed result to any even shard_bytes
 * (defect D6); a tail of shard_bytes % 64 bytes is coded as one more chunk in the
 * layout undoLastChunkEncoding implies (root.zig:338-348; the reference itself
 * panics on tails, root.zig:385). Caller owns every buffer. */

/* replaces `encode(allocator, original_count, recovery_count, original)` root.zig:14-30.
 * original[k] -> recovery_out[m] (each shard_bytes). */
int rs_encode(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
              const uint8_t *const *original, uint8_t *const *recovery_out);

/* replaces `decode(allocator, original_count, recovery_count, original, recovery)` root.zig:32-84.
 * original[i] / recovery[i] == NULL marks a missing shard. restored_out[k]
 * receives every original (present ones copied through, root.zig:76-81). */
int rs_decode(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
              const uint8_t *const *original, const uint8_t *const *recovery, uint8_t *const *restored_out);

/* ----------------------------------------- Encoder object (root.zig:86-174) */
typedef struct rs_encoder rs_encoder;
/* Encoder.init root.zig:94-122 */
int rs_encoder_new(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, rs_encoder **out);
/* Encoder.addOriginalShard root.zig:128-134 */
int rs_encoder_add_original_shard(rs_encoder *enc, const uint8_t *shard, size_t len);
/* Encoder.encode root.zig:136-173: recovery_out[m] receives borrowed pointers
 * valid until the next encode / rs_encoder_free. */
int rs_encoder_encode(rs_encoder *enc, const uint8_t **recovery_out);
/* Encoder.deinit root.zig:124-126 (resets for reuse: rs_encoder_reset) */
void rs_encoder_free(rs_encoder *enc);
int rs_encoder_reset(rs_encoder *enc);

/* ----------------------------------------- Decoder object (root.zig:176-336)
 * The reference keeps these methods private; exposed here with the same checks. */
typedef struct rs_decoder rs_decoder;
int rs_decoder_new(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, rs_decoder **out);
int rs_decoder_add_original_shard(rs_decoder *dec, uint64_t index, const uint8_t *shard, size_t len);
int rs_decoder_add_recovery_shard(rs_decoder *dec, uint64_t index, const uint8_t *shard, size_t len);
/* restored_out[k]: borrowed pointers to all k originals (supplied ones copied,
 * missing ones restored), valid until the next decode / rs_decoder_free. */
int rs_decoder_decode(rs_decoder *dec, const uint8_t **restored_out);
void rs_decoder_free(rs_decoder *dec);

/* -------------------------------------------- batched device entry points
 * Device-resident, asynchronous on `stream`, thread-safe, stateless apart
 * from a per-(k, m, flags[, erasure pattern]) plan cache. Stripes are
 * independent; shards of one stripe are contiguous (shard stride =
 * shard_bytes); a stripe stride of 0 means packed.
 *   d_original: [n_stripes][k][shard_bytes]  (stride original_stripe_stride)
 *   d_recovery: [n_stripes][m][shard_bytes]  (stride recovery_stripe_stride)
 * Alignment, for every entry point of this section: with shards of whole 64-byte chunks
 * (shard_bytes % 64 == 0) each device pointer and each stripe stride must be a multiple of
 * 4 bytes, else RS_ERR_INVALID_ARGUMENT and nothing is written (rs_verify_batch_dev: d_original
 * and its stride; its d_recovery may have any alignment). 16-byte alignment of all of them is
 * what the hipRTC kernels and the widest table kernels need, and what the rs_*_kernel_name
 * functions assume; a narrower layout computes the same bytes on the table kernels with
 * narrower lanes (_nv2 at 8 bytes, _nv1 at 4), as rs_last_kernels reports. Other shard sizes
 * (tails) run on aligned padded copies and take any alignment. tests/test_gpu_layouts.py. */
int rs_encode_batch_dev(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, uint64_t n_stripes,
                        const void *d_original, uint64_t original_stripe_stride, void *d_recovery,
                        uint64_t recovery_stripe_stride, uint32_t flags, rs_stream_t stream);

/* Reconstruct the missing originals of every stripe; one erasure pattern for
 * the whole batch. present: host array of k+m flags (originals, then
 * recovery). The slots of missing shards still lie inside the caller's rows of
 * d_original / d_recovery (the layout does not change), but their contents never
 * influence a result and they are never written: they may hold garbage, stale data or
 * another object's shards. The same holds for every reconstruct entry point below (per-stripe
 * patterns, host batches, rs_decode, the Decoder), and no input buffer is written at all
 * (tests/test_gpu_missing_slots.py checks it for every kernel family).
 *   d_restored: [n_stripes][e][shard_bytes], e = missing originals, ascending index.
 * Nothing else of d_restored is written (stride padding, rows past the batch). */
int rs_reconstruct_batch_dev(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                             uint64_t n_stripes, const uint8_t *present, const void *d_original,
                             uint64_t original_stripe_stride, const void *d_recovery,
                             uint64_t recovery_stripe_stride, void *d_restored, uint64_t restored_stripe_stride,
                             uint32_t flags, rs_stream_t stream);

/* Reconstruct with a per-stripe erasure pattern (§8f rank 2). d_present: DEVICE
 * array, n_stripes rows of k+m flags (row stride present_stride, 0 = k+m). The
 * erasure locator (Generic.zig:200-215) is evaluated per stripe on the GPU: a small
 * erased set's log terms are summed point by point, only large sets take the two
 * 64K-point FWHTs. Stripe s restores its missing originals, ascending, into
 * slots [0, e_s) of its d_restored row ([n][max_e][shard_bytes]); slots >= e_s
 * are not written. d_status (device, n int32, may be NULL) receives per stripe
 * RS_OK, RS_ERR_NOT_ENOUGH_SHARDS (< k present: no slot of the stripe's row is written)
 * or RS_ERR_INVALID_ARGUMENT (e_s > max_e: restored slots past max_e are dropped). Bytes
 * of a d_present row past its k+m flags are ignored. */
int rs_reconstruct_batch_dev_patterns(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                                      uint64_t n_stripes, const uint8_t *d_present, uint64_t present_stride,
                                      uint32_t max_e, const void *d_original, uint64_t original_stripe_stride,
                                      const void *d_recovery, uint64_t recovery_stripe_stride, void *d_restored,
                                      uint64_t restored_stripe_stride, int32_t *d_status, uint32_t flags,
                                      rs_stream_t stream);

/* Verify (scrub): for every stripe, compare each stored recovery shard with what
 * rs_encode_batch_dev (same k, m, shard_bytes, flags) would write for the stripe's originals.
 * Neither input is written. d_bad: device, n_stripes rows of m bytes (row stride bad_stride,
 * 0 = m): d_bad[s][r] = 1 if recovery shard r of stripe s differs in any byte, else 0. Every
 * one of the n*m flag bytes is written; bytes between rows are not touched. d_bad_count
 * (device, optional): receives the number of flags set.
 * Accepts everything the encode accepts (any even shard_bytes, 1 / 2 KiB shards, 4-byte
 * aligned buffers, low-rate codes, the quirk flags), always meaning "what the encode would
 * write", and validates in the encode's order (n_stripes == 0: RS_OK, nothing written; a NULL
 * pointer, a stride below the row size or 0 < bad_stride < m: RS_ERR_INVALID_ARGUMENT).
 * A set flag says that the stripe is inconsistent and which recovery rows disagree with the
 * originals: one corrupt recovery shard sets one flag; one corrupt original sets all m flags
 * under the corrected arithmetic (flags == 0), because every block of the encode is a
 * multiplication by a nonzero field element. Which shard is the corrupt one is
 * rs_locate_batch_dev's answer (below).
 * Slices of stripes are encoded into a scratch of at most RS_AMD_SCRATCH_CAP_MB (by the
 * encode's own kernels) and compared with the stored shards: k + 3m rows of traffic per stripe,
 * and no second parity buffer of the whole batch. */
int rs_verify_batch_dev(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, uint64_t n_stripes,
                        const void *d_original, uint64_t original_stripe_stride, const void *d_recovery,
                        uint64_t recovery_stripe_stride, uint8_t *d_bad, uint64_t bad_stride, uint64_t *d_bad_count,
                        uint32_t flags, rs_stream_t stream);
/* The path a verify takes: "<rs_encode_kernel_name>+verify_compare". */
const char *rs_verify_kernel_name(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes);

/* Locate (between scrub and heal): for every stripe, name the one shard whose corruption
 * explains every disagreement between the stored recovery shards and the originals. With
 * flags == 0 the encode is linear over GF(2^16), parity[r] = sum_j c[r][j] * original[j] with
 * every c[r][j] nonzero, so the syndromes S_r = encode(originals)[r] ^ stored[r] of one corrupt
 * original j are S_r = c[r][j] * err for every r: the ratio S_1 / S_0 at one nonzero symbol names
 * j (the k ratios c[1][j] / c[0][j] are distinct, the code being MDS), and
 * S_r == (c[r][j] / c[0][j]) * S_0 over the whole shard for every r >= 1 confirms it.
 * d_located (device, n_stripes int32, every one written): an index in [0, k + m), originals
 * first, then recovery (the order of `present`), or one of the values below.
 * d_present (device, optional): n_stripes rows of k + m flags (row stride present_stride, 0 =
 * k + m; bytes between rows are not touched): 1 for every shard except the located one;
 * RS_LOCATE_RECOVERY_SET: 0 at each disagreeing recovery shard; RS_LOCATE_CLEAN and
 * RS_LOCATE_UNLOCATED: all 1. A row can be passed as it is to rs_reconstruct_batch_dev_patterns
 * with max_e = 1: a corrupt original is restored from the other shards; a stripe whose bad
 * shards are recovery shards has e_s = 0 there and is healed by rs_rebuild_batch_dev (below), which
 * takes the same rows and puts back originals and recovery shards alike.
 * d_counts (device, optional): 4 words, the stripes that are clean, located to a single shard,
 * a recovery set, unlocated. Neither input buffer is written.
 * Guarantee: with at most one corrupt shard in a stripe and m >= 2 the answer is exact. With two
 * corrupt shards and m >= 3 no stripe is reported as a single shard (a weight-2 and a weight-1
 * error with equal syndromes would differ by a codeword of weight <= 3 < m + 1). With m == 2 two
 * corrupt shards can imitate one: the code's limit. m == 1: a disagreeing stripe is
 * RS_LOCATE_UNLOCATED. Locating more than one corrupt shard is rs_locate_multi_batch_dev's job
 * (below).
 * Accepts everything rs_verify_batch_dev accepts, validated in the same order and with the same
 * alignment contract (any even shard_bytes, d_original and its stride 4-byte aligned when
 * shard_bytes % 64 == 0, d_recovery at any alignment, low-rate codes, strides; n_stripes == 0:
 * RS_OK, nothing written; NULL d_located or 0 < present_stride < k + m:
 * RS_ERR_INVALID_ARGUMENT), except that flags must be 0, else RS_ERR_INVALID_ARGUMENT and
 * nothing is written: under RS_FLAG_QUIRK_D1 the engine's multiply is no field multiplication
 * (the syndromes of one error are not multiples of each other), and RS_FLAG_QUIRK_D2 leaves some
 * originals out of the parity altogether (k > chunk, k % chunk == 0), where no parity can name
 * them.
 * Slices of stripes (scratch at most RS_AMD_SCRATCH_CAP_MB, tables and flags included) are
 * encoded and compared as by rs_verify_batch_dev; stripes whose m rows all disagree are then read
 * once more, 2m rows, by the confirm kernel. */
#define RS_LOCATE_CLEAN (-1)        /* every recovery shard agrees */
#define RS_LOCATE_RECOVERY_SET (-2) /* 2..m-1 recovery shards disagree, at least one agrees: the originals are
                                       good, the disagreeing recovery shards are the bad ones */
#define RS_LOCATE_UNLOCATED (-3)    /* all m disagree and no single original explains it (or m == 1 and it disagrees) */
int rs_locate_batch_dev(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, uint64_t n_stripes,
                        const void *d_original, uint64_t original_stripe_stride, const void *d_recovery,
                        uint64_t recovery_stripe_stride, int32_t *d_located, uint8_t *d_present,
                        uint64_t present_stride, uint64_t *d_counts, uint32_t flags, rs_stream_t stream);
/* The path a locate takes: "<rs_encode_kernel_name>+verify_compare+locate". */
const char *rs_locate_kernel_name(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes);
/* Host check of the locate algebra (no device): the code's coefficient ratios are distinct, and
 * over `trials` random stripes of a few symbols per shard a corrupted original, a corrupted
 * recovery shard, two corrupted recovery shards and (m >= 3) two corrupted originals get the
 * answer the guarantee above states. *mismatches = wrong answers. RS_ERR_INVALID_ARGUMENT for
 * original_count == 0. */
int rs_locate_selftest(uint64_t original_count, uint64_t recovery_count, int trials, uint64_t seed,
                       uint64_t *mismatches);

/* Locate, several shards: for every stripe, name the up to max_t shards whose corruption explains
 * every disagreement, originals and recovery shards alike. With flags == 0 let G = [C | I_m], an
 * m x (k + m) matrix over GF(2^16): column j < k holds the encode's coefficients c[r][j], column
 * k + r the unit vector e_r (a corrupt recovery shard r disturbs only S_r). With corrupt shards T
 * the syndrome vector of symbol p is S(p) = sum_{i in T} G_i * err_i(p). Every symbol of a stripe
 * shares T, so the S(p) span a subspace V of dimension rho <= |T|; the code being MDS, any m columns
 * of G are independent, and the columns of G that lie in V are corrupt shards. The rank is found
 * by the pass that confirms it: a basis of V in reduced form grows by one vector per round, taken
 * at the first symbol the previous round found outside the span.
 * max_t: 1 .. min(recovery_count / 2, RS_LOCATE_MAX_T).
 * d_count (device, n_stripes int32, every one written): 0 for a clean stripe, t in [1, max_t] for
 * t located shards, or RS_LOCATE_UNLOCATED. RS_LOCATE_RECOVERY_SET is never returned: bad recovery
 * shards are named like any others.
 * d_located (device, optional): n_stripes rows of max_t int32 (row stride located_stride, in
 * words, 0 = max_t; words between rows are not touched): slots [0, t) hold the located shards'
 * indices in [0, k + m), ascending, originals first as in `present`; every other slot of the row
 * holds -1 (all of them for a clean or unlocated stripe).
 * d_present (device, optional): n_stripes rows of k + m flags (row stride present_stride, 0 =
 * k + m; bytes between rows are not touched): 0 at each located shard, 1 elsewhere; all 1 for
 * clean and unlocated stripes. A row can be passed as it is to rs_rebuild_batch_dev with
 * max_e = max_t.
 * d_counts (device, optional): max_t + 2 words, the stripes with 0, 1, .., max_t located shards,
 * then the unlocated ones. No input is written.
 * Guarantee, for max_t <= m / 2: a stripe with at most m / 2 corrupt shards is never given a wrong
 * answer. Its T is reported exactly if |T| <= max_t and the errors of its shards are linearly
 * independent as rows over the symbol positions (any real corruption, with overwhelming
 * probability); it is RS_LOCATE_UNLOCATED if the rank exceeds max_t, or if the errors are
 * rank-deficient (err_b = alpha * err_a at every symbol, or fewer distinct corrupt symbol positions
 * than shards): then fewer than rho columns lie in V and nothing is named. More than m / 2 corrupt
 * shards are beyond unique decoding: such a stripe is unlocated whenever its rank exceeds max_t, and
 * may otherwise imitate a smaller set. Out of scope: more than RS_LOCATE_MAX_T shards,
 * probabilistic location beyond m / 2, known erasures combined with errors, a *_host form, the
 * quirk flags.
 * Validated on the host before any device call, in rs_locate_batch_dev's order and with its
 * alignment contract (original_count == 0, the encode's checks, n_stripes == 0: RS_OK and nothing
 * written, NULL pointers and strides below the row size, flags != 0, d_original and its stride
 * 4-byte aligned when shard_bytes % 64 == 0), then RS_ERR_INVALID_ARGUMENT for a NULL d_count,
 * max_t == 0 or above min(recovery_count / 2, RS_LOCATE_MAX_T) (so recovery_count < 2 is always
 * invalid), 0 < located_stride < max_t, 0 < present_stride < k + m.
 * Slices of stripes (scratch at most RS_AMD_SCRATCH_CAP_MB: the encode's m rows, 98 * max_t * m
 * bytes of basis and multiply tables and m + 16 + 8 * max_t bytes of state per stripe) are encoded
 * and compared as by rs_verify_batch_dev, whose flags settle clean stripes; then max_t + 1 rounds of
 * k_mloc_check (16-byte, dword or byte loads as rs_last_kernels reports: _x16 / _x4 / _x1) and
 * k_mloc_extend, k_mloc_match and k_mloc_finish run without host synchronisation. A stripe with t
 * corrupt shards is read t + 1 more times, 2m rows each (round 0 reads only the rows whose compare
 * flag is set). */
#define RS_LOCATE_MAX_T 8
int rs_locate_multi_batch_dev(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                              uint64_t n_stripes, uint32_t max_t, const void *d_original,
                              uint64_t original_stripe_stride, const void *d_recovery,
                              uint64_t recovery_stripe_stride, int32_t *d_count, int32_t *d_located,
                              uint64_t located_stride, uint8_t *d_present, uint64_t present_stride,
                              uint64_t *d_counts, uint32_t flags, rs_stream_t stream);
/* The path it takes: "<rs_encode_kernel_name>+verify_compare+locate_multi_t<max_t>". */
const char *rs_locate_multi_kernel_name(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                                        uint32_t max_t);
/* Host check of the algebra above (no device), on 12 symbols per shard: over `trials` random
 * stripes, every t in 0 .. max_t corrupt shards (random mixes of originals and recovery shards,
 * errors of full rank) must be located exactly; max_t + 1 shards, each wrong at a symbol of its
 * own, and with recovery_count >= 4 a pair with proportional errors must be RS_LOCATE_UNLOCATED.
 * *mismatches = wrong answers (or 1 for a zero coefficient). RS_ERR_INVALID_ARGUMENT for
 * original_count == 0 or a max_t the batch call rejects. */
int rs_locate_multi_selftest(uint64_t original_count, uint64_t recovery_count, uint32_t max_t, int trials,
                             uint64_t seed, uint64_t *mismatches);

/* Update (the small write): some originals of a stripe change and its stored recovery shards
 * follow in place, without the other originals. With flags == 0 the encode is linear over
 * GF(2^16), parity[r] = sum_j c[r][j] * original[j], so changing original j from old to new
 * changes recovery shard r by exactly c[r][j] * (old ^ new): after the call d_recovery holds, byte
 * for byte, what rs_encode_batch_dev writes for the new originals (if it held that for the old
 * ones). 2u + 2m shard rows of traffic per stripe for u changed originals (u + 2m in delta form)
 * instead of the encode's k + m.
 * d_index (device): n_stripes rows of max_u words (row stride index_stride, in words; 0 =
 * max_u). Slot i of stripe s names the original that changed (< k) or holds RS_UPDATE_NONE; empty
 * slots may sit anywhere in a row, and a row of all RS_UPDATE_NONE leaves its stripe untouched.
 * d_old, d_new (device): [n_stripes][max_u][shard_bytes] with one stripe stride,
 * change_stripe_stride (0 = packed); slot i's shard is at s * stride + i * shard_bytes, and the
 * shards of empty slots are never read. d_old == NULL is the delta form: d_new already holds
 * old ^ new (what a node receives when the data lives elsewhere).
 * d_recovery (device): [n_stripes][m][shard_bytes], updated in place:
 * recovery[r] ^= sum_i c[r][index_i] * (old_i ^ new_i). No byte outside the m rows of a stripe is
 * written (stride padding, rows past the batch), and d_index, d_old and d_new are never written.
 * d_status (device, n_stripes int32, may be NULL; every entry written): RS_OK;
 * RS_ERR_INVALID_SHARD_INDEX if any slot is >= k and not RS_UPDATE_NONE (checked first);
 * RS_ERR_DUPLICATE_SHARD_INDEX if two slots name the same original. A stripe that is not RS_OK has
 * no byte of its parity written; the other stripes of the batch are updated.
 * Validated on the host before any device call, in this order: original_count == 0
 * (RS_ERR_TOO_FEW_ORIGINAL_SHARDS); the encode's checks of the counts and shard_bytes; n_stripes
 * == 0 or max_u == 0: RS_OK, nothing written; then RS_ERR_INVALID_ARGUMENT for a NULL d_index,
 * d_new or d_recovery, max_u > k, a stride below its row size, flags != 0 (as for
 * rs_locate_batch_dev: under RS_FLAG_QUIRK_D1 the multiply is no field multiplication, and
 * RS_FLAG_QUIRK_D2 leaves originals out of the parity), with shard_bytes % 64 == 0 a d_old, d_new,
 * d_recovery or stripe stride of theirs that is no multiple of 4, and a d_old or d_new range that
 * overlaps [d_recovery, d_recovery + n_stripes * stride) (the update would read what it writes).
 * Other shard sizes (tails) take any alignment, on byte accesses; low-rate codes are served.
 * Slices of stripes (scratch at most RS_AMD_SCRATCH_CAP_MB: 96 * max_u * m bytes of multiply
 * tables per stripe, built on the device) run k_update_prepare, then k_update_apply (16-byte,
 * dword or byte accesses by what every buffer, stride and shard_bytes allow, as rs_last_kernels
 * reports: _x16 / _x4 / _x1). Up to 4 changed originals of a stripe are applied in one pass over
 * its parity; every further 4 cost one more read and write of it. */
#define RS_UPDATE_NONE 0xFFFFFFFFu /* an empty slot of a d_index row */
int rs_update_batch_dev(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, uint64_t n_stripes,
                        uint32_t max_u, const uint32_t *d_index, uint64_t index_stride, const void *d_old,
                        const void *d_new, uint64_t change_stripe_stride, void *d_recovery,
                        uint64_t recovery_stripe_stride, int32_t *d_status, uint32_t flags, rs_stream_t stream);
/* Host check of the update algebra (no device): over `trials` random stripes of a few symbols per
 * shard, 1..min(max_u, k) distinct originals change and stored ^ sum c[r][j] * delta must equal
 * the scalar encode of the new originals. *mismatches = wrong symbols (or 1 for a zero
 * coefficient). RS_ERR_INVALID_ARGUMENT for original_count == 0. */
int rs_update_selftest(uint64_t original_count, uint64_t recovery_count, uint32_t max_u, int trials, uint64_t seed,
                       uint64_t *mismatches);

/* Rebuild (heal): every lost shard of a stripe comes back, recovery shards included, each stripe
 * with its own set of lost shards. What a node or disk failure under rotated parity needs: the
 * failed node held a data shard of some stripes and a parity shard of others.
 * d_present (device): the rows of rs_reconstruct_batch_dev_patterns (k + m flags per stripe, row
 * stride present_stride, 0 = k + m), so rs_locate_batch_dev's d_present rows can be passed as they
 * are. For stripe s let E be its missing originals, ascending (e_o of them), Q its missing recovery
 * shards, ascending (e_r), e_s = e_o + e_r.
 * d_rebuilt (device): [n_stripes][max_e][shard_bytes] (stripe stride rebuilt_stripe_stride, 0 =
 * packed). Slots [0, e_o) of the stripe's row receive the originals E, slots [e_o, e_s) the
 * recovery shards Q, byte for byte what rs_encode_batch_dev writes for the stripe's true
 * originals. Slots >= e_s are not written, nothing past max_e slots is written, no input is
 * written, and the contents of missing slots never influence a result.
 * d_status (device, n_stripes int32, may be NULL; every entry written): RS_OK (a stripe with
 * nothing missing too: nothing of it is written); RS_ERR_NOT_ENOUGH_SHARDS with fewer than k shards
 * present (e_s > m): nothing of the stripe is written; RS_ERR_INVALID_ARGUMENT with e_s > max_e: the
 * first max_e slots in the order above are written, as rs_reconstruct_batch_dev_patterns does.
 * Validated on the host before any device call, in this order: original_count == 0
 * (RS_ERR_TOO_FEW_ORIGINAL_SHARDS); the encode's checks of the counts and shard_bytes; n_stripes
 * == 0 or max_e == 0: RS_OK, nothing written; then RS_ERR_INVALID_ARGUMENT for a NULL d_present,
 * d_original, d_recovery or d_rebuilt, max_e > m, a stride below its row size, flags != 0 (as for
 * rs_locate_batch_dev and rs_update_batch_dev: under RS_FLAG_QUIRK_D1 and RS_FLAG_QUIRK_D2 a lost
 * recovery shard is no linear function of the syndromes), with shard_bytes % 64 == 0 a data pointer
 * or stripe stride that is no multiple of 4, and a d_rebuilt range that overlaps either input range.
 * Accepts everything rs_reconstruct_batch_dev_patterns accepts with flags == 0: tails, any even
 * shard_bytes, 4- and 8-byte-aligned layouts, wide and low-rate codes, strides.
 * Two forms. Fast: codes with k <= 256, m <= 8 on whole 4 KiB units with
 * 16-byte-aligned buffers and strides run one pass of the code's syndrome network
 * (rs_psyn_rebuild_k<k>_m<m>_<hash>, hipRTC) after k_psyn_rebuild_plan: k + e_s shard rows of
 * traffic per stripe. While that kernel compiles in the background (larger codes; RS_AMD_JIT_SYNC=1
 * compiles in the caller) a call takes the general form; rs_last_kernels reports what ran.
 * General, everything else, in slices of stripes (scratch at most RS_AMD_SCRATCH_CAP_MB, at least
 * one stripe): the per-stripe reconstruct into slots [0, e_o), k_rebuild_gather of the stripe's
 * originals into a scratch, the encode of that scratch, k_rebuild_pick of rows Q: about
 * 3k + m + e_o + 2 e_r rows per stripe. It is the correct-everywhere path, not the fast one.
 * Out of scope: rebuilding in place into the missing slots, a *_host form, a batch-wide-pattern
 * form with compiled-in patterns, a fused wide-code form. */
int rs_rebuild_batch_dev(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, uint64_t n_stripes,
                         const uint8_t *d_present, uint64_t present_stride, uint32_t max_e,
                         const void *d_original, uint64_t original_stripe_stride,
                         const void *d_recovery, uint64_t recovery_stripe_stride,
                         void *d_rebuilt, uint64_t rebuilt_stripe_stride, int32_t *d_status,
                         uint32_t flags, rs_stream_t stream);
/* The path a rebuild is planned to take: "psyn_rebuild_k<k>_m<m>" (the fast form, given aligned
 * buffers), else "<rs_patterns_kernel_name>+rebuild_gather+<rs_encode_kernel_name>+rebuild_pick". */
const char *rs_rebuild_kernel_name(uint64_t k, uint64_t m, size_t shard_bytes, uint32_t max_e);
/* Generate the rebuild variant of the code's syndrome network and compile it for gfx950 with
 * hipRTC (no device). RS_ERR_INVALID_ARGUMENT where the code has no such kernel (k > 256, m > 8,
 * low rate). */
int rs_rebuild_compile_check(uint64_t k, uint64_t m, double *compile_ms, uint64_t *code_bytes);
/* Host check of the rebuild algebra (no device): k_psyn_rebuild_plan's coefficients on scalar
 * symbols, over `trials` random stripes of a few symbols per shard with random sets of lost shards
 * (among them recovery shards only, originals only and e_s = m), the missing slots poisoned; the
 * rebuilt symbols must equal the data and the scalar encode. *mismatches = wrong symbols (or 1 for
 * a zero coefficient or a singular block). RS_ERR_INVALID_ARGUMENT for original_count == 0. */
int rs_rebuild_selftest(uint64_t k, uint64_t m, int trials, uint64_t seed, uint64_t *mismatches);

/* -------------------------------------- host-resident batches (end to end)
 * Same layouts and semantics as the *_dev calls, but the batch lives in HOST
 * memory: the library streams it through HBM in slices on a 2-slot
 * H2D -> kernel -> D2H pipeline on its own streams (PCIe full duplex overlapped
 * with compute) and returns when the results are in host memory. Pinned host
 * buffers (hipHostMalloc / hipHostRegister / torch pin_memory) run at PCIe rate;
 * pageable buffers are copied by host threads through the ring's own pinned staging.
 * A reconstruct reads only the present shards: one copy per run of consecutive present
 * rows, in slices of 256 MiB widened up to 1 GiB while the narrowest run's copy would
 * move less than 8 MiB. Ring copies use the 2D copy form (faster than the 1D one from
 * pinned memory). The ring's device buffers persist per device. Knobs: Environment, below. */
int rs_encode_batch_host(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, uint64_t n_stripes,
                         const void *h_original, uint64_t original_stripe_stride, void *h_recovery,
                         uint64_t recovery_stripe_stride, uint32_t flags);
int rs_reconstruct_batch_host(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                              uint64_t n_stripes, const uint8_t *present, const void *h_original,
                              uint64_t original_stripe_stride, const void *h_recovery,
                              uint64_t recovery_stripe_stride, void *h_restored, uint64_t restored_stripe_stride,
                              uint32_t flags);

/* The same host-memory batches split over several GPUs of the node: device i of
 * devices[0..n_devices) (NULL = every visible device) takes the contiguous stripe
 * range [i*n/D, (i+1)*n/D) and runs it on its own worker thread and staging ring
 * (stripes are independent: no exchange between devices). Returns the first
 * failing device's status (its message in rs_last_error) after every worker ended. */
int rs_encode_batch_host_multi(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                               uint64_t n_stripes, const void *h_original, uint64_t original_stripe_stride,
                               void *h_recovery, uint64_t recovery_stripe_stride, uint32_t flags,
                               const int *devices, int n_devices);
int rs_reconstruct_batch_host_multi(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                                    uint64_t n_stripes, const uint8_t *present, const void *h_original,
                                    uint64_t original_stripe_stride, const void *h_recovery,
                                    uint64_t recovery_stripe_stride, void *h_restored,
                                    uint64_t restored_stripe_stride, uint32_t flags, const int *devices,
                                    int n_devices);

/* Which device kernel a call would run on in its steady state ("net_encode_i10_o4",
 * "encode_reg_w4_nv4", "decode_matrix_e4_nv4", "encode_generic_nv1",
 * "net_fft_encode_i200_o55", "net_fft_pdecode_i200_o55", ...), assuming 16-byte aligned
 * buffers. present: k+m flags as for rs_reconstruct_batch_dev, or NULL for "the first
 * min(k, m) originals lost". net_<role>_* = bit-sliced XOR network (or bit-sliced FFT
 * kernel, net_fft_*) generated for the plan and compiled with hipRTC on first use (shards of
 * 1 / 2 KiB or whole 4 KiB units, <= 64 outputs; up to 64 input blocks compile in the call,
 * larger maps in the background). A prediction: the kernels a
 * call actually launched are in rs_last_kernels. */
const char *rs_encode_kernel_name(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes);
const char *rs_reconstruct_kernel_name(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                                       const uint8_t *present);
/* Path rs_reconstruct_batch_dev_patterns takes for these arguments (16-byte aligned
 * buffers): "psyn_k<k>_m<m>" (k <= 256, m <= 8, whole 4 KiB units: the code's syndrome
 * network + a per-stripe solve), "fft_decode" (chunk 16 / 32 / 64 codes with max_e >= 0.6 m,
 * or shards of whole 2 KiB units: the fused FFT reconstruct with per-stripe decode blocks
 * built on the GPU), "fft_syndromes+psyn_solve" (chunk 16 / 32 / 64 otherwise: FFT syndromes
 * with per-stripe masks + the e x e solve in output groups of 8), "pattern_matrix"
 * (per-stripe e x k table matrices, W <= 32, max_e <= 8) or "pattern_fft" (the reference's
 * decode on the generic FFT kernels: D1, D2-dropping codes, everything else) or
 * "pattern_fft_low" (low-rate codes: the same decode in the low-rate layout). These are
 * what a call is planned to run; rs_last_kernels reports what it did run. */
const char *rs_patterns_kernel_name(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes,
                                    uint32_t max_e, uint32_t flags);

/* Per-pattern kernels of wide codes compile in a background thread. A wide-code pattern's
 * first calls run the fused FFT reconstruct with the pattern as data (rs_fft_decode_*,
 * nothing compiled per pattern). One steady-state kernel per pattern is then built on the
 * background worker, behind the full plan's build: a network where one beats the fused
 * kernel (few losses: the direct map, queued at the pattern's second call; without the fused
 * reconstruct: the e x e syndrome map), else the fused kernel with the pattern compiled in
 * (rs_fft_pdecode_*, k <= 256; RS(200,55): 8-16 s of hipRTC), queued at the pattern's
 * second call. The pattern-compiled kernels are bounded: at most 32 patterns per code and
 * device (later patterns keep the pattern-as-data kernel), and none is queued while more
 * than 2 jobs wait on the worker (a later call retries). The calls run the first form until
 * the steady-state kernel is loaded. rs_net_wait blocks until the worker is idle (no plan
 * build or compile queued or running): after two calls + rs_net_wait the next call runs the
 * pattern's steady-state kernel (rs_reconstruct_warm gets there at once). The counts are
 * knobs: Environment, below. Returns RS_OK. */
int rs_net_wait(void);

/* Drive one erasure pattern of rs_reconstruct_batch_dev (same arguments) to its steady
 * state without running a batch: build its full plan and compile and load every kernel
 * its calls will launch, blocking until done. The next call runs the steady-state kernel
 * (check with rs_last_kernels). */
int rs_reconstruct_warm(uint64_t original_count, uint64_t recovery_count, size_t shard_bytes, const uint8_t *present,
                        uint32_t flags);

/* The kernels the calling thread's most recent compute call (the *_dev, *_host, one-shot,
 * Encoder/Decoder and engine entry points) launched, in launch order, ';'-separated,
 * consecutive repeats collapsed: hipRTC kernels by symbol (rs_net_encode_i10_o4_<hash>,
 * rs_fft_decode_k200_m55_..., the names rocprofv3 reports), precompiled ones by their
 * rs_*_kernel_name form (encode_reg_w4_nv4, k_erasure_logs, ...). Host batches launch on
 * worker threads and are recorded there, not here. Valid until the thread's next call. */
const char *rs_last_kernels(void);

/* ------------------------------------------------ fault injection (tests only)
 * The reference runs its encode under std.testing.checkAllAllocationFailures
 * (tests.zig:131-156): every allocation of the call fails in turn and must surface as
 * error.OutOfMemory with nothing leaked. Here every allocation the library makes — plan
 * objects, device and stream-ordered buffers, pinned staging — is counted; after
 * rs_debug_fail_alloc(n) the n-th one (from 0, all threads) fails as if out of memory and
 * the call returns RS_ERR_OUT_OF_MEMORY. n < 0 disarms. Returns the number of allocations
 * counted since the previous rs_debug_fail_alloc call. */
int64_t rs_debug_fail_alloc(int64_t n);
/* Drop every cache holding device or pinned memory (plans, device tables, staging rings,
 * pooled one-shot contexts; compiled kernels stay loaded), after any background plan build
 * finished. *pooled_contexts (optional) = one-shot contexts left in the pool (0). */
int rs_debug_release_caches(uint64_t *pooled_contexts);
/* Host erasure locators (root.zig:277-289, Generic.zig:200-215 evalPoly): the library sums a
 * small erased set's log terms point by point instead of the two 65536-point transforms.
 * Evaluates both for `received` (high rate: recovery at [0, m), originals at [C, C + k),
 * C = ceilPow2(m); low != 0: rs_gf.hpp erasure_logs_low's layout) and returns the number of
 * positions below ceilPow2(C + k) (low: ceilPow2(C + m)) where they differ mod 65535; -1 on
 * invalid arguments. Host only, no device. */
int64_t rs_debug_erasure_logs_check(uint64_t k, uint64_t m, const uint8_t *received, int low);
/* Measurement builds of the FFT kernels (rs_fftnet.cpp debug_of, bit 6): every wave
 * of workgroup 0 stamps s_memtime around each barrier of its third unit; copies the current
 * device's 8 x 64 stamps (wave-major) to out[0, min(n, 512)). */
int rs_debug_fft_stamps(uint64_t *out, uint64_t n);

/* hipRTC activity of this process: kernels compiled, code objects found in the on-disk
 * cache, modules loaded. Any pointer may be NULL. */
int rs_jit_stats(uint64_t *compiles, uint64_t *cache_hits, uint64_t *modules);

/* Plan-time network kernel: generate the bit-sliced network of an encode (present
 * == NULL) or of one reconstruct pattern and compile it with hipRTC for gfx950, without
 * loading it (no device needed: a build check). *compile_ms (optional) = compile time.
 * RS_ERR_INVALID_ARGUMENT if the shape has no network form, RS_ERR_DEVICE if hipRTC fails. */
int rs_net_compile_check(uint64_t original_count, uint64_t recovery_count, const uint8_t *present,
                         uint32_t flags, double *compile_ms);

/* Generate the per-stripe syndrome-network reconstruct kernels of
 * rs_reconstruct_batch_dev_patterns (rs_psyn.hpp) and compile them with hipRTC (no
 * device): for k <= 256, m <= 8 the code's fixed k -> m syndrome network plus the
 * per-stripe e x e solve; for chunk 16 / 32 / 64 codes the FFT syndrome kernel with
 * per-stripe masks plus the generic solve. RS_ERR_INVALID_ARGUMENT if the code has none. */
int rs_psyn_compile_check(uint64_t original_count, uint64_t recovery_count, uint32_t flags, double *compile_ms,
                          uint64_t *code_bytes);
/* Bit-sliced FFT encode kernel (wide codes, chunk 32 / 64): generate
 * it for (original_count, recovery_count, flags) and compile it with hipRTC, without
 * loading it (a build check; no device needed). Optional outputs: compile time, code
 * object bytes, and the generated kernel's VALU instruction estimate per 2 KiB unit
 * (all waves). RS_ERR_INVALID_ARGUMENT if the code has no such kernel. */
int rs_fft_compile_check(uint64_t original_count, uint64_t recovery_count, uint32_t flags, double *compile_ms,
                         uint64_t *code_bytes, uint64_t *valu_ops);
/* Host check of that kernel's arithmetic (its butterfly schedule with its (u, v)
 * coordinate matrices on scalar symbols, against the codec's scalar encode, with
 * the data shards flagged in skip (k bytes, NULL = none) read as zero): *mismatches
 * = wrong parity symbols over `trials` random stripes. */
int rs_fft_selftest(uint64_t original_count, uint64_t recovery_count, uint32_t flags, const uint8_t *skip,
                    int trials, uint64_t *mismatches);

/* Fused FFT reconstruct of wide codes (replaces the reference's
 * Decoder.decode, root.zig:268-335, for chunk 16 / 32 / 64 codes, corrected multiply):
 * the syndromes of e recovery rows and the erasure-locator decode in one kernel, the
 * pattern as data. rs_fft_decode_compile_check generates and compiles it (no device);
 * rs_fft_decode_selftest runs its schedule on scalar symbols (host) for `trials` random
 * stripes losing e originals (and random surplus recovery shards) against the data:
 * *mismatches = wrong restored symbols. RS_ERR_INVALID_ARGUMENT if the code has no such
 * kernel or e > recovery_count. */
int rs_fft_decode_compile_check(uint64_t original_count, uint64_t recovery_count, double *compile_ms,
                                uint64_t *code_bytes);
/* The same kernel with one erasure pattern compiled in (present: k + m flags): the locator
 * scalars as constant multiplies, rows, blocks and outputs static (the steady state of a
 * pattern reused across batches). RS_ERR_NOT_ENOUGH_SHARDS if the pattern cannot decode. */
int rs_fft_pdecode_compile_check(uint64_t original_count, uint64_t recovery_count, const uint8_t *present,
                                 double *compile_ms, uint64_t *code_bytes);
int rs_fft_decode_selftest(uint64_t original_count, uint64_t recovery_count, uint32_t erased, int trials,
                           uint64_t *mismatches);

/* Host check of the low-rate reconstruct's algebra (no device): `trials` random stripes
 * of one symbol per shard, encoded by the low-rate encode, lose 1..min(k, m) random
 * originals plus random recovery shards (>= k present), and are restored by the
 * erasure-locator decode in the low-rate layout (rs_lowrate.cpp). *mismatches = wrong
 * restored symbols. RS_ERR_INVALID_ARGUMENT for a high-rate code. */
int rs_lowrate_selftest(uint64_t original_count, uint64_t recovery_count, int trials, uint64_t seed,
                        uint64_t *mismatches);

/* ---------------------------------------- Engine seam (Generic.zig), test shim
 * The reference's comptime Engine interface (root.zig:10-12) at per-call
 * granularity, run on the GPU over a HOST buffer of shard_count shards of
 * shard_bytes (copied in and out). For stage-by-stage parity only. */
int rs_engine_fft(uint8_t *shards, uint64_t shard_count, size_t shard_bytes, uint64_t pos, uint64_t size,
                  uint64_t truncated_size, uint64_t skew_delta, uint32_t flags);  /* Generic.zig:15 */
int rs_engine_ifft(uint8_t *shards, uint64_t shard_count, size_t shard_bytes, uint64_t pos, uint64_t size,
                   uint64_t truncated_size, uint64_t skew_delta, uint32_t flags); /* Generic.zig:80 */
int rs_engine_mul_scalar(uint8_t *chunks, size_t bytes, uint16_t log_m, uint32_t flags); /* Generic.zig:220 */
/* Generic.zig:200 evalPoly over 65536 u16 erasure flags, in place (host FWHT). */
int rs_engine_eval_poly(uint16_t *erasures, uint64_t truncated_size);

/* ---------------------------------------------------- tables (tables.zig) */
const uint16_t *rs_table_exp(void);       /* [65536] */
const uint16_t *rs_table_log(void);       /* [65536] */
const uint16_t *rs_table_skew(void);      /* [65535] */
const uint16_t *rs_table_log_walsh(void); /* [65536] */
/* tables.zig:94-118 `mul_128: [65536]Lut`, `Lut = [2][4]u128`: for multiplier log_m, byte
 * [log_m][h][i][j] = byte h (0 low, 1 high) of mul16(j << 4i, log_m) — the x86 engine's
 * pshufb nibble tables (8 MiB, built on the first call; the GPU kernels use their own
 * v_perm / bit-sliced forms). NULL if it cannot be allocated. */
const uint8_t *rs_table_mul_128(void);

/* ------------------------------------------------------------------ Environment
 * The variables a user of the library may set (the public rows of the table in
 * csrc/rs_env.hpp, which lists every variable read). Each is read at every use, so a change
 * takes effect on the next call. Unset or empty means the default. A number outside its
 * range is clamped to it. A flag is off only for a number equal to 0 and on for any other
 * value.
 *   RS_AMD_CACHE_DIR
 *       directory of the on-disk code-object cache; empty: no disk cache; unset:
 *       $XDG_CACHE_HOME/rs_amd or ~/.cache/rs_amd
 *   RS_AMD_FDEC
 *       0: never the fused FFT reconstruct; 1: whenever it applies, and no pattern-
 *       compiled kernels; anything else: auto
 *   RS_AMD_HOST_SLICE_MB (1.., default computed)
 *       input MiB per host-batch slice; unset: 256, and reconstructs widen it for narrow
 *       row runs
 *   RS_AMD_HOST_SLOTS (1..8, default 2)
 *       slices in flight in the host-batch ring
 *   RS_AMD_HOST_STAGE (flag, default on)
 *       0: pageable host buffers go to the runtime as they are, without the ring's
 *       pinned staging
 *   RS_AMD_HOST_THREADS (1..64, default computed)
 *       host threads of the staging copies; unset: min(16, hardware threads)
 *   RS_AMD_JIT (flag, default on)
 *       0: no hipRTC kernels at all, every call runs on the precompiled table kernels
 *   RS_AMD_JIT_CACHE_MAX (0.., default 1024)
 *       loaded hipRTC modules per process; past it new maps run on the table kernels
 *   RS_AMD_JIT_SYNC (flag, default off)
 *       1: background compiles run in the calling thread instead
 *   RS_AMD_JIT_VERBOSE
 *       set at all: report every compile and disk-cache hit on stderr
 *   RS_AMD_LOW_BLOCK (flag, default on)
 *       0: low-rate reconstructs keep the W-point decode instead of the block form
 *   RS_AMD_PDEC (flag, default on)
 *       0: no pattern-compiled fused reconstruct kernels
 *   RS_AMD_PDEC_AFTER (1.., default 2)
 *       a pattern is compiled in on its n-th use
 *   RS_AMD_PDEC_MAX (0.., default 32)
 *       pattern-compiled kernels per code and device
 *   RS_AMD_PDEC_QUEUE (0.., default 2)
 *       pattern compiles waiting on the worker before new ones are put off
 *   RS_AMD_PLAN_CACHE (1.., default 4096)
 *       plans kept per kind before the least recently used are dropped
 *   RS_AMD_SCRATCH_CAP_MB (1.., default 2048)
 *       scratch MiB per launch of the generic kernels */

#ifdef __cplusplus
}
#endif
#endif /* REEDSOL_AMD_H */
