/* fec_hip_ragged.h — ragged forms of fec_rs_verify_batch and fec_rs_reconstruct_some_batch (fec_hip.h):
 * block b's shards are block_len[b] bytes long, as in the ragged encode, reconstruct and recover of
 * fec_hip.h ("Ragged forms of ..."). With them the whole klauspost Encoder surface (Encode, Verify,
 * Reconstruct, ReconstructData, ReconstructSome) takes ragged batches. Part of lib0xfec_hip's C ABI;
 * conventions (return codes, layouts, alignment, stream order, the sticky error word and fec_sync())
 * are those of fec_hip.h. */
#ifndef FEC_HIP_RAGGED_H
#define FEC_HIP_RAGGED_H

#include "fec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Common to both calls, as for the ragged calls of fec_hip.h.
 *
 * FEC_DEVICE only: any other `flags` value returns FEC_ERR_INVALID_ARG. block_len is an array of
 * nblocks uint32 in device memory, 4-byte aligned (else FEC_ERR_ALIGNMENT). Shard layout, strides and
 * alignment are those of the uniform calls, checked with max_shard_len in place of shard_len
 * (shard_stride >= max_shard_len; every slot readable over shard_stride bytes). max_shard_len == 0
 * returns FEC_ERR_SHARD_NO_DATA, max_shard_len > 2^30 FEC_ERR_INVALID_ARG. The host-side checks run in
 * the uniform call's order (shard counts, k + m against the call's limit, flags, max_shard_len, the
 * ctx and its code, nblocks == 0, then the pointers, block_len among them, the layouts and the word
 * alignment). Batches are cut into launches as the uniform calls cut them, with max_shard_len as the
 * shard length. All three matrix kinds are served, as by the uniform calls (fec_hip_matrix.h).
 *
 *   0 < block_len[b] <= max_shard_len   the block gets exactly what the uniform call gives for that
 *                                       block alone with shard_len = block_len[b]; nothing at or past
 *                                       round_up(len, 16) of any slot is read or written
 *   block_len[b] == 0                   no byte of the block is read or written
 *   block_len[b] > max_shard_len        the block is neither read nor written; its status is
 *                                       FEC_ERR_SHARD_SIZE, and fec_sync() returns FEC_ERR_SHARD_SIZE
 *                                       unless something that ranks before it is pending
 *
 * The kernels' work and memory traffic follow the sum of the blocks' lengths (in 16-byte chunks), not
 * nblocks times the longest. */

/* Verify, ragged: k + m <= 256. block_status (required) receives per block
 *   1                   bytes [0, block_len[b]) of every parity shard equal what the encode writes from
 *                       the block's data; also a block of length 0, and every block when m == 0
 *   0                   some parity byte below block_len[b] differs
 *   FEC_ERR_SHARD_SIZE  block_len[b] > max_shard_len (not counted)
 * The tail chunk is compared under the block's own byte mask: bytes at and past block_len[b] of a slot,
 * data or parity, never matter. mismatch_count (optional; one uint32 in device memory, 4-byte
 * aligned) receives the exact number of blocks with status 0. A mismatch does not touch the sticky
 * word: fec_sync() returns FEC_OK after a batch with bad blocks.
 * m == 0 comes before every per-block rule, the oversize one included: a code without parity has
 * nothing to compare, block_len is not read, every status is 1 (also where block_len[b] >
 * max_shard_len), the count is 0 and the sticky word is not touched. */
int fec_rs_verify_ragged_batch(fec_ctx *ctx, int k, int m, size_t max_shard_len, size_t nblocks,
                               const uint8_t *data, size_t data_block_stride,
                               const uint8_t *parity, size_t parity_block_stride,
                               size_t shard_stride, const uint32_t *block_len,
                               int32_t *block_status, uint32_t *mismatch_count, int flags);

/* Reconstruct / ReconstructSome, ragged, in place: k + m <= FEC_MAX_DECODE_SHARDS, one uint32 present
 * mask and an optional want mask per block (want_mask NULL: every shard), shard strides below 2^32
 * (else FEC_ERR_INVALID_ARG). Statuses (block_status optional) and the sticky word are what
 * fec_rs_reconstruct_some_batch gives for the same masks: 0, FEC_ERR_TOO_FEW_SHARDS, or
 * FEC_ERR_SINGULAR under a custom code; they do not depend on the length, but for the oversize
 * override above. Every wanted missing shard of a block that can be rebuilt, data or parity, receives
 * bytes [0, len) and zeros over [len, round_up(len, 16)) in its own slot; a failing block has no byte
 * written. With m == 0 the parity region is neither read nor written and may be NULL. */
int fec_rs_reconstruct_some_ragged_batch(fec_ctx *ctx, int k, int m, size_t max_shard_len, size_t nblocks,
                                         uint8_t *data, size_t data_block_stride,
                                         uint8_t *parity, size_t parity_block_stride,
                                         size_t shard_stride, const uint32_t *present_mask,
                                         const uint32_t *want_mask, const uint32_t *block_len,
                                         int32_t *block_status, int flags);

#ifdef __cplusplus
}
#endif

#endif /* FEC_HIP_RAGGED_H */
