/* fec_hip_some_wide.h — wide reconstruct-some: fec_rs_reconstruct_some_batch (fec_hip.h) for codes of
 * up to FEC_MAX_WIDE_SHARDS shards. Part of lib0xfec_hip's C ABI; conventions (return codes, layouts,
 * alignment, stream order, the sticky error word and fec_sync()) are those of fec_hip.h. */
#ifndef FEC_HIP_SOME_WIDE_H
#define FEC_HIP_SOME_WIDE_H

#include "fec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* RS Reconstruct / ReconstructSome, in place, for every code the encode takes: the contract of
 * fec_rs_reconstruct_some_batch with masks in the wide calls' form. Missing data AND parity shards of
 * a block are rebuilt, and a want mask chooses which. It is the call that heals what
 * fec_rs_locate_batch, fec_rs_locate_multi_batch and fec_rs_locate_partial_batch report for codes of
 * more than 32 shards: their present_out masks go straight into present_mask.
 *
 * Masks. Block b's present mask, and its want mask if given, are the mask_words words at
 * present_mask + b*mask_words and want_mask + b*mask_words; shard i is bit i % 32 of word i / 32.
 * Bits at and above k + m of either mask are ignored. want_mask == NULL means "every shard" (klauspost
 * Reconstruct). Both are device memory, 4-byte aligned (else FEC_ERR_ALIGNMENT), and only read.
 *
 * Per block, with R = the shards below k + m that are missing and wanted:
 *   R empty                              the block is untouched, status 0, even with fewer than k
 *                                        shards present
 *   R non-empty, fewer than k present    the block is untouched, status FEC_ERR_TOO_FEW_SHARDS; the
 *                                        code is sticky and fec_sync() reports it once
 *   otherwise                            every shard in R, data or parity, is rebuilt into its own
 *                                        slot from the first k present shards in index order; status 0
 * A rebuilt shard's slot receives bytes [0, shard_len) and zeros over [shard_len, round_up(shard_len,
 * 16)); nothing else is written anywhere, missing shards outside R included. Each shard is the value
 * of one polynomial of degree < k at the shard's index, so a rebuilt parity shard is byte for byte what
 * fec_rs_encode_batch writes from the block's data, and a want mask naming only data shards gives
 * exactly the bytes and statuses of fec_rs_reconstruct_wide_batch. block_status (optional) is nblocks
 * int32 in device memory, 4-byte aligned. With m == 0 the parity region is neither read nor written
 * and may be NULL.
 *
 * Limits: k >= 1, m >= 0, k + m <= FEC_MAX_WIDE_SHARDS; FEC_MASK_WORDS(k + m) <= mask_words <= 8, else
 * FEC_ERR_INVALID_ARG. FEC_DEVICE only: any other `flags` value returns FEC_ERR_INVALID_ARG. A shard
 * stride of 2^32 or more returns FEC_ERR_INVALID_ARG. The host-side checks run in the locate calls'
 * order: shard counts, k + m > 256, flags, shard_len (0: FEC_ERR_SHARD_NO_DATA, above 2^30:
 * FEC_ERR_INVALID_ARG), mask_words, the ctx, nblocks == 0 (FEC_OK, nothing touched), null pointers
 * (present_mask, data, and parity when m > 0), the layouts, the word alignment of present_mask,
 * block_status and want_mask.
 *
 * With k + m <= FEC_MAX_DECODE_SHARDS and mask_words == 1 the call is fec_rs_reconstruct_some_batch,
 * bytes and errors unchanged (as the two wide decode calls forward to their narrow forms).
 *
 * Cost. One wave per block turns the masks into a record of |R| x k coefficient bytes (a record has
 * room for max(m, 1) rows), then the rebuild of fec_rs_reconstruct_wide_batch runs over the records,
 * output rows in passes of 16. The records live in the ctx's workspace; batches are cut into launches
 * as the wide decode cuts them. */
int fec_rs_reconstruct_some_wide_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                                       uint8_t *data, size_t data_block_stride,
                                       uint8_t *parity, size_t parity_block_stride,
                                       size_t shard_stride,
                                       const uint32_t *present_mask, const uint32_t *want_mask,
                                       size_t mask_words, int32_t *block_status, int flags);

#ifdef __cplusplus
}
#endif

#endif /* FEC_HIP_SOME_WIDE_H */
