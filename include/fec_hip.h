/*
 * fec_hip.h — C ABI of the MI355X (gfx950) FEC codec: lib0xfec_hip.so
 *
 * This is the device boundary of the reference's hot path. In ddritzenhoff/0xFEC the
 * block codes live in package internal/fec and their arithmetic is a Go call into
 * github.com/klauspost/reedsolomon v1.12.4 (go.mod:24). This library replaces that
 * arithmetic with hand-written HIP kernels; the Go side keeps its block bookkeeping and
 * binds these entry points through cgo. Signatures use only plain
 * pointers and sizes.
 *
 *   entry point                 replaces (reference file:line)
 *   --------------------------  ---------------------------------------------------------
 *   fec_rs_prepare              reedsolomon.New(k, m)       internal/fec/reed_solomon.go:16,
 *                                                           internal/fec/manager.go:60,83
 *   fec_rs_encode_batch         Encoder.Encode(shards)      internal/fec/reed_solomon.go:51
 *   fec_rs_reconstruct_batch    Encoder.ReconstructData     internal/fec/reed_solomon.go:124
 *   fec_rs_recover_batch        ReconstructData + the copy-out of recoverSymbolPayloads
 *                                                           internal/fec/reed_solomon.go:124-133
 *   fec_rs_reconstruct_wide_batch, fec_rs_recover_wide_batch
 *                               the same two for every code klauspost accepts (k + m <= 256),
 *                               present masks of 1..8 words per block
 *   fec_rs_encode_ragged_batch, fec_rs_reconstruct_ragged_batch, fec_rs_recover_ragged_batch
 *                               Encode / ReconstructData / the copy-out for a batch whose blocks
 *                               each have their own shard length, as the reference's blocks do
 *                               (2 + biggestSourceSymbolLenSoFar, reed_solomon.go:47,80)
 *   fec_rs_verify_ragged_batch, fec_rs_reconstruct_some_ragged_batch (fec_hip_ragged.h)
 *                               Verify and Reconstruct / ReconstructSome for such a batch: with them the
 *                               whole Encoder surface takes a shard length per block
 *   fec_rs_verify_batch         Encoder.Verify(shards), batched: one verdict per block (klauspost's
 *                               interface; the reference does not call it)
 *   fec_rs_locate_batch         no counterpart: which shard of a block that fails Verify is the corrupt
 *                               one (klauspost's advice is to leave out each shard in turn, reconstruct
 *                               and verify again), and the present mask that heals the block
 *   fec_rs_locate_multi_batch   no counterpart: up to m/2 corrupt shards of a block that fails Verify, the
 *                               radius of the code, and the present mask that heals the block (m <= 16)
 *   fec_rs_locate_partial_batch no counterpart: the same for a block that also has missing shards, to the
 *                               radius (m - e) / 2 that its e missing shards leave; the present mask
 *                               then rebuilds the missing and the corrupt shards in one go (m <= 16)
 *   fec_rs_reconstruct_some_batch
 *                               Encoder.Reconstruct (want_mask NULL) and Encoder.ReconstructSome, in
 *                               place: missing parity shards are rebuilt too (klauspost's interface;
 *                               the reference calls ReconstructData only)
 *   fec_rs_update_batch         Encoder.Update(shards, newDatashards), batched: parity repaired from the
 *                               old and new versions of a block's changed data shards alone (klauspost's
 *                               interface; the reference does not call it)
 *   fec_rs_encode_idx_batch     Encoder.EncodeIdx(dataShard, idx, parity), batched and for any set of
 *                               columns per call: parity accumulates as data shards arrive (klauspost's
 *                               interface; the streaming sender's block fill, manager.go:123-158)
 *   fec_xor_encode_batch        xorScheme.xor loop          internal/fec/xor.go:28-33,44-56
 *   fec_xor_reconstruct_batch   xorScheme recover loops     internal/fec/xor.go:80-86
 *
 * Shard layout (all entry points). A batch is `nblocks` independent blocks of k data and m
 * parity shards. Data shard j of block b lives at  data + b*data_block_stride + j*shard_stride,
 * parity shard i at  parity + b*parity_block_stride + i*shard_stride; each is `shard_len`
 * bytes long. One interleaved [block][k+m][shard_stride] array is the special case
 * parity = data + k*shard_stride, parity_block_stride = data_block_stride. Shards are
 * (the reference's shard = payload | zero pad | big-endian uint16 length, i.e.
 * biggest+2 bytes: reed_solomon.go:70-89, xor.go:44-56). Bytes [0, shard_len) of every
 * output shard receive the result; with FEC_DEVICE, bytes [shard_len, round_up(shard_len,
 * 16)) of an output shard slot are also written, as zeros (whole 16-byte stores), and
 * nothing past that is touched. FEC_HOST writes exactly shard_len bytes per output.
 *
 * Distances (FEC_DEVICE). Strides and offsets are 64-bit throughout: the block strides, the
 * distance between any two regions (data, parity, out, old data; parity may lie below the data)
 * and a block's or shard's offset from its base may be any value that the alignment rules admit,
 * beyond 2^32 included; the regions of one call need not lie in one allocation. One limit: the
 * calls that rebuild shards (fec_rs_reconstruct_batch, fec_rs_recover_batch, their wide and ragged
 * forms, fec_rs_reconstruct_some_batch and its forms) take shard strides below 2^32 and return
 * FEC_ERR_INVALID_ARG for a shard_stride of 2^32 or more, before anything is enqueued. Every other
 * call takes any shard stride.
 *
 * Memory kinds (`flags`):
 *   FEC_DEVICE  pointers are device memory of the ctx's device; shard_stride, block
 *               strides and base pointers must be multiples of 16, every shard slot
 *               (shard_stride bytes) must be readable; present_mask and block_status must be
 *               4-byte aligned (the kernels read masks by 4-byte scalar loads, which drop the
 *               low two address bits). The call is asynchronous on the
 *               ctx stream; per-block decode failures are reported through `block_status`
 *               (if given) and, sticky, by fec_sync().
 *   FEC_HOST    pointers are host memory with any layout; the ctx stages the batch
 *               through pinned buffers (H2D -> kernel -> D2H) and returns when done. Chunks
 *               of the batch alternate between two staging sets on two streams, so staging,
 *               transfers and kernels of neighbouring chunks overlap; only the shards the code
 *               needs cross PCIe (encode: k up, m down; reconstruct: the data shards and the
 *               parity planes the blocks read up, the rebuilt shards down).
 *   FEC_HOST_PINNED  as FEC_HOST, but the caller's buffers are pinned (hipHostMalloc) or
 *               registered (hipHostRegister): no staging copies, each shard column moves with
 *               one 2D DMA between the caller's layout and the device. fec_rs_recover_batch
 *               is FEC_DEVICE only.
 *
 * Shard limits. Encode takes every code klauspost accepts, k + m <= 256. The narrow decode calls
 * (fec_rs_reconstruct_batch, fec_rs_recover_batch, fec_xor_reconstruct_batch) take one uint32
 * present mask per block and so k + m <= FEC_MAX_DECODE_SHARDS = 32; they run the tuned kernels.
 * The wide decode calls take FEC_MASK_WORDS(k + m)..8 mask words per block and decode every code
 * the library encodes, k + m <= FEC_MAX_WIDE_SHARDS = 256. A wide call with k + m <= 32 and one
 * mask word is forwarded to the narrow call. The ragged calls follow the uniform ones: encode
 * k + m <= 256, reconstruct and recover k + m <= 32; of those in fec_hip_ragged.h,
 * fec_rs_verify_ragged_batch k + m <= 256 and fec_rs_reconstruct_some_ragged_batch k + m <= 32.
 *
 * Threading: a ctx has one HIP stream and is used by one caller at a time (the
 * reference's manager is per connection and not thread-safe either: manager.go:41-48).
 * Use one ctx per device per host thread.
 */
#ifndef FEC_HIP_H
#define FEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes: 0 on success, negative on failure. */
#define FEC_OK 0
#define FEC_ERR_INVALID_ARG (-1)     /* null pointer, bad stride/length/flags */
#define FEC_ERR_INV_SHARD_NUM (-2)   /* klauspost ErrInvShardNum: k <= 0 or m < 0 */
#define FEC_ERR_MAX_SHARD_NUM (-3)   /* klauspost ErrMaxShardNum: k + m > 256 (narrow decode: > 32) */
#define FEC_ERR_TOO_FEW_SHARDS (-4)  /* klauspost ErrTooFewShards */
#define FEC_ERR_SHARD_SIZE (-5)      /* klauspost ErrShardSize; ragged calls: block_len[b] > max_shard_len */
#define FEC_ERR_SHARD_NO_DATA (-6)   /* klauspost ErrShardNoData: shard_len == 0 */
#define FEC_ERR_ALIGNMENT (-7)       /* FEC_DEVICE layout not 16-byte aligned, or a mask / status
                                        array not 4-byte aligned */
#define FEC_ERR_HIP (-8)             /* HIP runtime failure */
#define FEC_ERR_NOMEM (-9)
#define FEC_ERR_NO_DEVICE (-10)
#define FEC_ERR_SINGULAR (-11)       /* klauspost errSingular: the rows of the first k present shards of a
                                        custom code matrix are dependent (fec_hip_matrix.h) */
#define FEC_ERR_NO_MATRIX (-12)      /* kind FEC_MATRIX_CUSTOM: no matrix registered for this (k, m), or a
                                        call that custom matrices do not serve (fec_hip_matrix.h) */

#define FEC_DEVICE 0
#define FEC_HOST 1
#define FEC_HOST_PINNED 2

/* Largest n = k + m the narrow reconstruct calls accept (their present masks are one uint32). */
#define FEC_MAX_DECODE_SHARDS 32
/* Largest n = k + m the wide reconstruct calls accept, and the mask words a code of n shards needs. */
#define FEC_MAX_WIDE_SHARDS 256
#define FEC_MASK_WORDS(n) (((n) + 31) / 32)          /* 1..8 */

typedef struct fec_ctx fec_ctx;

/* Library / device. */
const char *fec_version(void);
const char *fec_strerror(int code);
int fec_device_count(int *count);

/* Context: device binding, one HIP stream, cached code matrices, workspace, pinned staging. */
int fec_ctx_create(int device, fec_ctx **out);
void fec_ctx_destroy(fec_ctx *ctx);
/* Run subsequent work on an external hipStream_t (NULL = the device's null stream). Work the
 * ctx already queued on its previous stream is ordered before the new stream's (an event wait,
 * no host sync), since both share the ctx's workspace. */
int fec_ctx_set_stream(fec_ctx *ctx, void *hip_stream);
/* Go back to the ctx-owned stream. */
int fec_ctx_reset_stream(fec_ctx *ctx);
void *fec_ctx_stream(fec_ctx *ctx);
/* Free the host-path staging (FEC_HOST / FEC_HOST_PINNED: kHostSets = 3 sets of pinned host and
 * device buffers, each up to one 128 MiB chunk of input plus its outputs, kept by the ctx between
 * calls so that a stream of calls does not re-register memory) after the ctx's host-path work
 * has finished. The next host-path call allocates them again. No reference counterpart (the
 * reference codes in Go memory); INTEGRATION.md lists the per-ctx footprint. */
int fec_ctx_release_staging(fec_ctx *ctx);
/* Wait for the ctx stream. Returns FEC_ERR_TOO_FEW_SHARDS if any FEC_DEVICE reconstruct
 * since the last fec_sync met a block with fewer than k present shards, or
 * FEC_ERR_INVALID_ARG if a recover met a block with more erasures than output slots, or
 * FEC_ERR_SHARD_SIZE if a ragged call met a block longer than its max_shard_len and neither of
 * the other two happened, or FEC_ERR_SINGULAR if a decode under a custom matrix met a block whose
 * rows are dependent and nothing else happened (then clears it). */
int fec_sync(fec_ctx *ctx);

/* The n x k systematic matrix of RS(k, m) (n = k + m), row-major, host memory. No device
 * needed. Same matrix as klauspost reedsolomon.New(k, m) with default options. */
int fec_rs_matrix(int k, int m, uint8_t *out);

/* Validate (k, m) and cache the code on the ctx (klauspost New). Optional: the batch calls
 * prepare on first use. */
int fec_rs_prepare(fec_ctx *ctx, int k, int m);

/* RS encode: parity shard i of each block = XOR_j M[k+i][j] * data shard j. */
int fec_rs_encode_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                        const uint8_t *data, size_t data_block_stride,
                        uint8_t *parity, size_t parity_block_stride,
                        size_t shard_stride, int flags);

/* RS ReconstructData, in place. present_mask[b] bit i set <=> shard i of block b present
 * (shards 0..k-1 data, k..k+m-1 parity; n = k + m <= 32). For each block, every missing DATA
 * shard is rebuilt, into its own slot, from the first k present shards in index order;
 * missing parity shards are not touched; a block with no missing data shard is untouched.
 * block_status (optional, same memory kind as the masks) receives 0 or
 * FEC_ERR_TOO_FEW_SHARDS per block. FEC_HOST: returns FEC_ERR_TOO_FEW_SHARDS if any block
 * failed (the other blocks are still rebuilt). */
int fec_rs_reconstruct_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                             uint8_t *data, size_t data_block_stride,
                             const uint8_t *parity, size_t parity_block_stride,
                             size_t shard_stride, const uint32_t *present_mask,
                             int32_t *block_status, int flags);

/* Out-of-place RS recovery: the device form of reedSolomonScheme.recoverSymbolPayloads
 * (internal/fec/reed_solomon.go:92-136), whose result is the erased source payloads in
 * ascending shard order. For block b the e erased data shards are rebuilt (same arithmetic
 * as fec_rs_reconstruct_batch) into  out + b*out_block_stride + r*shard_stride, r = 0..e-1,
 * in ascending shard order; data and parity are only read. out_slots = shard slots per block
 * in `out`. block_status (optional) receives e (>= 0) or FEC_ERR_TOO_FEW_SHARDS, or
 * FEC_ERR_INVALID_ARG when e > out_slots (that block is not written). An out slot is an output
 * shard slot like any other: slots r < e of a block that succeeds receive bytes [0, shard_len)
 * and zeros up to round_up(shard_len, 16); slots r >= e, the slots of a block that fails or has
 * nothing erased, and every byte outside the slots' first round_up(shard_len, 16) bytes are not
 * touched. FEC_DEVICE only; fec_sync() reports any failed block. */
int fec_rs_recover_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                         const uint8_t *data, size_t data_block_stride,
                         const uint8_t *parity, size_t parity_block_stride,
                         size_t shard_stride, const uint32_t *present_mask,
                         uint8_t *out, size_t out_block_stride, int out_slots,
                         int32_t *block_status, int flags);

/* Wide forms of the two calls above: k >= 1, m >= 0, k + m <= FEC_MAX_WIDE_SHARDS. Block b's
 * present mask is the mask_words words at present_mask + b*mask_words; shard i is present iff bit
 * i % 32 of word i / 32 is set; bits at and above k + m are ignored. FEC_MASK_WORDS(k + m) <=
 * mask_words <= 8, else FEC_ERR_INVALID_ARG. Everything else is as in the narrow calls: layout and
 * alignment rules, whole-16-byte-chunk outputs with zero fill, every missing data shard rebuilt
 * from the first k present shards in index order, missing parity and complete blocks untouched,
 * statuses (0 / e, FEC_ERR_TOO_FEW_SHARDS, FEC_ERR_INVALID_ARG for e > out_slots) and the sticky
 * word fec_sync() reports. With k + m <= 32 and mask_words == 1 the call is forwarded to the narrow
 * one; every other call runs the wide kernels (a plan record of up to ~16.5 KiB per block, then a
 * tiled rebuild). Reconstruct takes FEC_DEVICE and FEC_HOST (FEC_HOST_PINNED is treated as
 * FEC_HOST); its host form is plain, not pipelined: slices of the batch are staged whole through
 * pinned memory, rebuilt on the device and the rebuilt shards copied back, so it is PCIe-bound (it
 * exists for the scheme layer's one-block recoveries). Recover is FEC_DEVICE only. */
int fec_rs_reconstruct_wide_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                                  uint8_t *data, size_t data_block_stride,
                                  const uint8_t *parity, size_t parity_block_stride,
                                  size_t shard_stride, const uint32_t *present_mask, size_t mask_words,
                                  int32_t *block_status, int flags);
int fec_rs_recover_wide_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                              const uint8_t *data, size_t data_block_stride,
                              const uint8_t *parity, size_t parity_block_stride,
                              size_t shard_stride, const uint32_t *present_mask, size_t mask_words,
                              uint8_t *out, size_t out_block_stride, int out_slots,
                              int32_t *block_status, int flags);

/* Ragged forms of fec_rs_encode_batch, fec_rs_reconstruct_batch and fec_rs_recover_batch: block b's
 * shards are block_len[b] bytes long instead of one shard_len for the batch, and the kernels' work
 * and memory traffic follow the sum of the blocks' lengths (in 16-byte chunks), not nblocks times the
 * longest. FEC_DEVICE only: any other `flags` value returns FEC_ERR_INVALID_ARG.
 *
 * Layout and alignment. block_len is an array of nblocks uint32 in device memory, 4-byte aligned
 * (else FEC_ERR_ALIGNMENT). Shard layout, strides and alignment are those of the uniform calls and
 * are checked the same way with max_shard_len in place of shard_len (shard_stride >= max_shard_len;
 * every slot readable over shard_stride bytes). max_shard_len == 0 returns FEC_ERR_SHARD_NO_DATA,
 * max_shard_len > 2^30 FEC_ERR_INVALID_ARG. Encode takes k + m <= 256, the decode pair
 * k + m <= FEC_MAX_DECODE_SHARDS with one uint32 present mask per block. The host-side checks run in
 * the uniform calls' order (shard counts, flags, max_shard_len, out_slots, then the pointers,
 * block_len among them, the layouts and the word alignment). Batches are cut into launches as the
 * uniform calls cut them, with max_shard_len as the shard length.
 *
 * A block with 0 < block_len[b] <= max_shard_len is coded exactly as the uniform call would code it
 * alone with shard_len = block_len[b]: bytes [0, len) of each output shard receive the result, bytes
 * [len, round_up(len, 16)) are written as zeros, nothing else is written, and nothing at or past
 * round_up(len, 16) of any input slot is read.
 *
 * A block with block_len[b] == 0 has no byte read or written; its status is what its mask gives.
 *
 * Statuses and the sticky word are what the uniform call gives for the same masks (reconstruct: 0
 * or FEC_ERR_TOO_FEW_SHARDS; recover: e, FEC_ERR_TOO_FEW_SHARDS, or FEC_ERR_INVALID_ARG when
 * e > out_slots); they do not depend on the length. The encode's block_status (optional) receives 0.
 * (An encode with m == 0 or nblocks == 0 returns FEC_OK and does nothing, as the uniform one.)
 *
 * A block with block_len[b] > max_shard_len (a device-side value no host check can see) is neither
 * read nor written; its status is FEC_ERR_SHARD_SIZE, whatever its mask, and fec_sync() returns
 * FEC_ERR_SHARD_SIZE unless a too-few-shards or too-few-slots block is pending, which come first
 * (the sticky word still records what the block's mask gives). */
int fec_rs_encode_ragged_batch(fec_ctx *ctx, int k, int m, size_t max_shard_len, size_t nblocks,
                               const uint8_t *data, size_t data_block_stride,
                               uint8_t *parity, size_t parity_block_stride,
                               size_t shard_stride, const uint32_t *block_len,
                               int32_t *block_status, int flags);
int fec_rs_reconstruct_ragged_batch(fec_ctx *ctx, int k, int m, size_t max_shard_len, size_t nblocks,
                                    uint8_t *data, size_t data_block_stride,
                                    const uint8_t *parity, size_t parity_block_stride,
                                    size_t shard_stride, const uint32_t *present_mask,
                                    const uint32_t *block_len, int32_t *block_status, int flags);
int fec_rs_recover_ragged_batch(fec_ctx *ctx, int k, int m, size_t max_shard_len, size_t nblocks,
                                const uint8_t *data, size_t data_block_stride,
                                const uint8_t *parity, size_t parity_block_stride,
                                size_t shard_stride, const uint32_t *present_mask,
                                const uint32_t *block_len,
                                uint8_t *out, size_t out_block_stride, int out_slots,
                                int32_t *block_status, int flags);

/* RS Verify, batched: block_status[b] = 1 if bytes [0, shard_len) of every parity shard of block b
 * equal what fec_rs_encode_batch would write there from block b's data shards, else 0. Bytes at and
 * past shard_len of a slot, data or parity, never influence the result (the tail chunk of a shard
 * whose length is no multiple of 16 is compared under a byte mask), so the slots may hold anything
 * there. Nothing but block_status and mismatch_count is written; data and parity are only read.
 *
 * Every code the encode takes: k >= 1, m >= 0, k + m <= 256; with m == 0 every status is 1 and the
 * count 0. block_status (required) is nblocks words of device memory; mismatch_count (optional) is
 * one device uint32: when the call's work completes on the stream it holds the exact number of
 * blocks with status 0 (each bad block counted once). The call sets it; the caller need not clear
 * it. Both are 4-byte aligned (else FEC_ERR_ALIGNMENT). A mismatch is a result, not an error: it
 * does not touch the sticky word, and fec_sync() returns FEC_OK after it.
 *
 * FEC_DEVICE only: any other `flags` value returns FEC_ERR_INVALID_ARG. There is no host-resident
 * form: it would move k + m shards per block over the host link to learn one bit per block, which a
 * CPU encoder does faster where the shards already are. Layout and alignment rules are the uniform
 * calls'; the host-side checks run in their order (shard counts, flags, shard_len, ctx and code,
 * nblocks == 0 returns FEC_OK and touches nothing, then the pointers, the layouts and the word
 * alignment). Batches are cut into launches as the encode cuts them. */
int fec_rs_verify_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                        const uint8_t *data, size_t data_block_stride,
                        const uint8_t *parity, size_t parity_block_stride,
                        size_t shard_stride, int32_t *block_status,
                        uint32_t *mismatch_count, int flags);

/* Locate the corrupt shard of a block that fails verify. All k + m shards of a block are given (no
 * erasures); only bytes [0, shard_len) of each slot count. A block is consistent if its parity equals
 * what fec_rs_encode_batch would write from its data. bad_shard[b] receives
 *   FEC_LOCATE_CLEAN    the block is consistent
 *   s in [0, k + m)     the block is not consistent, m >= 2, and replacing the contents of shard s
 *                       alone (data for s < k, parity s - k otherwise) can make it consistent; at most
 *                       one such s exists, because the code has distance m + 1 >= 3
 *   FEC_LOCATE_UNKNOWN  the block is not consistent and no single shard explains it; with m == 1
 *                       every inconsistent block (one parity row cannot tell the shards apart)
 * With m == 0 every block is clean. One corrupt shard, any bytes of it, is always located when
 * m >= 2; t corrupt shards with 2 <= t < m always give FEC_LOCATE_UNKNOWN; with t >= m a wrong shard
 * can be named, as by any decoder past its distance.
 *
 * Outputs, all device memory, 4-byte aligned (else FEC_ERR_ALIGNMENT); the call sets every word of
 * each, the caller need not clear them:
 *   bad_shard    (required) nblocks verdicts
 *   present_out  (optional) nblocks x mask_words words in the wide calls' bit order: bits [0, k + m)
 *                set, except bit s of a located block; bits at and above k + m zero. With k + m <= 32
 *                and mask_words == 1 it is the present_mask with which fec_rs_reconstruct_some_batch
 *                rebuilds exactly the located shard, data or parity; for wider codes that of
 *                fec_rs_reconstruct_some_wide_batch (fec_hip_some_wide.h), which does the same.
 *                FEC_MASK_WORDS(k + m) <= mask_words <= 8, else FEC_ERR_INVALID_ARG, whether or not
 *                present_out is given
 *   counts       (optional) two uint32: when the call's work completes on the stream, [0] holds the
 *                located blocks and [1] the unknown ones
 * Nothing else is written; data and parity are only read, and bytes at and past shard_len of a slot
 * never influence a verdict. A corrupt block is a result, not an error: the sticky word is untouched
 * and fec_sync() returns FEC_OK.
 *
 * Every code the encode takes: k >= 1, m >= 0, k + m <= 256. FEC_DEVICE only: any other `flags` value
 * returns FEC_ERR_INVALID_ARG. Layout and alignment rules are the uniform calls'; the host-side
 * checks run in their order: shard counts, k + m > 256, flags, shard_len (0: FEC_ERR_SHARD_NO_DATA,
 * above 2^30: FEC_ERR_INVALID_ARG), mask_words, the ctx, nblocks == 0 (FEC_OK, nothing touched), null
 * pointers (bad_shard, data, and parity when m > 0), the layouts, the word alignment.
 *
 * Cost. A clean batch is read once per pass and no atomic is issued, as by fec_rs_verify_batch; a
 * pass takes parity row 0 and 15 further rows (verify: 16 rows), so codes of m > 16 read row 0 again
 * in each pass and some of them (m = 32, 47, 48, ...) take one pass more than verify.
 *
 * fec_rs_locate_multi_batch (below) names up to m / 2 corrupt shards of a block. */
#define FEC_LOCATE_CLEAN (-1)
#define FEC_LOCATE_UNKNOWN (-2)
int fec_rs_locate_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                        const uint8_t *data, size_t data_block_stride,
                        const uint8_t *parity, size_t parity_block_stride,
                        size_t shard_stride, int32_t *bad_shard,
                        uint32_t *present_out, size_t mask_words,
                        uint32_t *counts, int flags);

/* Locate up to m / 2 corrupt shards of a block that fails verify: fec_rs_locate_batch to the radius
 * of the code, which has distance m + 1. Regions, layouts, alignment rules and FEC_DEVICE-only are
 * those of fec_rs_locate_batch: all k + m shards of a block are given and only bytes [0, shard_len)
 * of each slot count.
 *
 * Let T = min(max_bad, m / 2). Per block b, let E_b be the smallest set of shards, |E_b| <= T, such
 * that replacing bytes [0, shard_len) of the shards in E_b alone can make the block consistent. If
 * such a set exists it is unique (two would differ by a nonzero codeword of weight <= 2 T <= m), and
 * it is the union, over byte columns, of the supports of each column's unique error vector of weight
 * <= T. bad_count[b] receives
 *   0                   the block is consistent
 *   |E_b| in [1, T]     E_b exists
 *   FEC_LOCATE_UNKNOWN  otherwise; with m <= 1 (T = 0) every inconsistent block
 * With m == 0 every block is 0. t corrupt shards with t <= T are always located exactly; with
 * T < t <= m - T the block is always unknown; with t > m - T a wrong set can be named, as by any
 * decoder past its distance: the result is always the smallest explaining set of at most T shards if
 * one exists, which past the radius need not be the shards that were changed. With max_bad == 1 the results agree with fec_rs_locate_batch block for
 * block: clean with 0, shard s with count 1 and bit s cleared, unknown with unknown.
 *
 * Outputs, all device memory, 4-byte aligned (else FEC_ERR_ALIGNMENT); the call sets every word of
 * each, the caller need not clear them:
 *   bad_count    (required) nblocks results
 *   present_out  (optional) nblocks x mask_words words in the wide calls' bit order: bits [0, k + m)
 *                set, less the bits of E_b; an unknown block keeps all k + m bits, so that healing
 *                leaves it untouched; bits at and above k + m zero. These are the masks that heal
 *                through fec_rs_reconstruct_some_batch (k + m <= 32, mask_words == 1) or
 *                fec_rs_reconstruct_some_wide_batch (fec_hip_some_wide.h; any k + m), located parity
 *                shards included. FEC_MASK_WORDS(k + m) <= mask_words <= 8, else
 *                FEC_ERR_INVALID_ARG, whether or not present_out is given
 *   counts       (optional) two uint32: when the call's work completes on the stream, [0] holds the
 *                located blocks (count >= 1) and [1] the unknown ones
 * Nothing else is written; a corrupt block is a result, not an error: the sticky word is untouched.
 * The call is stream-ordered like its siblings; its scratch memory (one bit per 16-byte chunk column
 * of a block and FEC_MASK_WORDS(k + m) + 1 words per block) is the ctx's workspace.
 *
 * Scope: k >= 1, 0 <= m <= 16, k + m <= 256. m > 16 is not yet supported and returns
 * FEC_ERR_INVALID_ARG, checked right after k + m; max_bad outside [1, FEC_LOCATE_MAX_BAD] returns
 * FEC_ERR_INVALID_ARG, checked after shard_len and before mask_words. The other host-side checks come
 * in fec_rs_locate_batch's order.
 *
 * Cost. A clean batch is read once, no atomic is issued and nothing is written but the outputs; a
 * bitmap clear and one launch over the bitmap come on top of fec_rs_locate_batch's work. Only the
 * chunks that hold a nonzero syndrome are read again and solved, one lane per chunk: a batch with
 * many corrupt chunks takes several times fec_rs_locate_batch's time.
 *
 * fec_rs_locate_partial_batch (below) takes blocks that also have missing shards. */
#define FEC_LOCATE_MAX_BAD 8
int fec_rs_locate_multi_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                              const uint8_t *data, size_t data_block_stride,
                              const uint8_t *parity, size_t parity_block_stride,
                              size_t shard_stride, int max_bad, int32_t *bad_count,
                              uint32_t *present_out, size_t mask_words,
                              uint32_t *counts, int flags);

/* Locate corrupt shards in blocks that also have missing shards: fec_rs_locate_multi_batch with a
 * present mask per block. Regions, layouts, alignment rules and FEC_DEVICE-only are those of
 * fec_rs_locate_multi_batch; only bytes [0, shard_len) of each present shard's slot count, and the
 * contents of a missing shard's slot never influence any output (no byte of it is read).
 *
 *   present_mask  (required) device memory, 4-byte aligned: block b's mask is mask_words words in the
 *                 wide calls' bit order (bit i % 32 of word i / 32 set: shard i is present); bits at
 *                 and above k + m are ignored
 *   mask_words    strides present_mask and present_out alike; FEC_MASK_WORDS(k + m) <= mask_words <= 8,
 *                 else FEC_ERR_INVALID_ARG
 *
 * Per block b let e_b be the number of clear bits below k + m and T_b = min(max_bad, (m - e_b) / 2) its
 * radius. The present shards of a block form a code of distance m - e_b + 1. bad_count[b] receives
 *   FEC_LOCATE_TOO_FEW   e_b > m: fewer than k shards are present; the block's shards are not examined
 *   0                    some codeword agrees with every present shard over bytes [0, shard_len). With
 *                        e_b == m this is vacuous: any k shards determine a codeword
 *   |E_b| in [1, T_b]    E_b is the smallest set of present shards, |E_b| <= T_b, whose replacement
 *                        alone makes the present shards consistent; it is unique (m - e_b + 1 > 2 T_b)
 *                        and is the union over byte columns of each column's unique error vector of
 *                        weight <= T_b
 *   FEC_LOCATE_UNKNOWN   the present shards are inconsistent and no such set exists; with T_b == 0
 *                        every inconsistent block
 * t corrupt present shards with t <= T_b are always located exactly; with T_b < t <= (m - e_b) - T_b the
 * block is always unknown; beyond that a wrong set can be named: the result is always the smallest
 * explaining set of at most T_b present shards if one exists, which past the radius need not be the
 * shards that were changed. max_bad lies in [0,
 * FEC_LOCATE_MAX_BAD]; 0 makes the call a verify of blocks with missing shards (results 0, unknown or
 * too few). With every mask full and max_bad >= 1 the results, masks and counts[0..1] are those of
 * fec_rs_locate_multi_batch block for block, and counts[2] is 0.
 *
 * Outputs, all device memory, 4-byte aligned (else FEC_ERR_ALIGNMENT); the call sets every word of
 * each:
 *   bad_count    (required) nblocks results
 *   present_out  (optional) nblocks x mask_words words: the block's present bits below k + m, less the
 *                bits of E_b for a located block, unchanged for every other block; bits at and above
 *                k + m zero. It may be the same pointer as present_mask (exact aliasing only: the
 *                masks are then updated in place); any other overlap is undefined. These masks go
 *                straight into fec_rs_reconstruct_some_batch (k + m <= 32, mask_words == 1) or
 *                fec_rs_reconstruct_some_wide_batch (fec_hip_some_wide.h; any k + m), which rebuilds
 *                the missing and the located shards, data and parity, in one go:
 *                e_b + |E_b| <= m leaves k shards present
 *   counts       (optional) three uint32: when the call's work completes on the stream, [0] holds the
 *                located blocks, [1] the unknown ones, [2] those with too few shards
 * Nothing else is written. A result is not an error: the sticky word is untouched and fec_sync()
 * returns FEC_OK after any mix of results. The scratch memory (fec_rs_locate_multi_batch's, and one
 * word and m 32-byte tables per block) is the ctx's workspace.
 *
 * Scope: k >= 1, 0 <= m <= 16, k + m <= 256. The host-side checks come in fec_rs_locate_multi_batch's
 * order: shard counts, k + m > 256, m > 16, flags, shard_len, max_bad, mask_words, the ctx,
 * nblocks == 0 (FEC_OK, nothing touched), null pointers (bad_count, present_mask, data, and parity when
 * m > 0), the layouts, the word alignment of the four word arrays. */
#define FEC_LOCATE_TOO_FEW (-3)
int fec_rs_locate_partial_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                                const uint8_t *data, size_t data_block_stride,
                                const uint8_t *parity, size_t parity_block_stride,
                                size_t shard_stride, const uint32_t *present_mask, size_t mask_words,
                                int max_bad, int32_t *bad_count, uint32_t *present_out,
                                uint32_t *counts, int flags);

/* RS Reconstruct / ReconstructSome, in place: as fec_rs_reconstruct_batch (k + m <=
 * FEC_MAX_DECODE_SHARDS, one uint32 present mask per block), but missing PARITY shards are rebuilt
 * as well, and a want mask chooses which missing shards. want_mask is one uint32 per block in
 * device memory, 4-byte aligned, or NULL for "every shard" (klauspost Reconstruct). Block b rebuilds
 * the shards  R = ~present_mask[b] & want_mask[b] & low_mask(k + m); bits at and above k + m of
 * either mask are ignored.
 *   R empty                              the block is untouched, status 0
 *   R non-empty, fewer than k present    the block is untouched, status FEC_ERR_TOO_FEW_SHARDS, and
 *                                        fec_sync() reports it as for the narrow call
 *   otherwise                            every shard in R, data or parity, is rebuilt into its own
 *                                        slot from the first k present shards in index order; status 0
 * A rebuilt shard's slot receives bytes [0, shard_len) and zeros up to round_up(shard_len, 16);
 * nothing else is written anywhere, missing shards outside R included. Each shard is the value of
 * one polynomial of degree < k at the shard's index, so a rebuilt parity shard is byte for byte
 * what fec_rs_encode_batch writes from the block's data. A want mask naming only data shards
 * (low_mask(k)) gives exactly the bytes and statuses of fec_rs_reconstruct_batch, by a plainer
 * route than that call's tuned kernels. FEC_DEVICE only (any other `flags` value returns
 * FEC_ERR_INVALID_ARG); the host-side checks are those of fec_rs_reconstruct_batch, with parity
 * required when m > 0. */
int fec_rs_reconstruct_some_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                                  uint8_t *data, size_t data_block_stride,
                                  uint8_t *parity, size_t parity_block_stride,
                                  size_t shard_stride, const uint32_t *present_mask,
                                  const uint32_t *want_mask, int32_t *block_status, int flags);

/* RS Update and EncodeIdx, batched: parity is changed in place from some of a block's data shards,
 *   parity_i ^= XOR over j in C_b of M[k+i][j] * delta_j,     i = 0..m-1,
 * where C_b is the set of columns j < k named by block b's mask, and delta_j is old_j ^ new_j
 * (fec_rs_update_batch: data shard j changed from its old to its new version) or data_j
 * (fec_rs_encode_idx_batch: data shard j is added to a parity that did not hold it yet).
 *
 * Masks. Block b's column mask is the mask_words words at mask + b*mask_words; column j is bit j % 32
 * of word j / 32 (the wide calls' form); bits at and above k are ignored. FEC_MASK_WORDS(k) <=
 * mask_words <= 8, else FEC_ERR_INVALID_ARG: the bound follows k, not k + m. The masks are device
 * memory, 4-byte aligned (else FEC_ERR_ALIGNMENT).
 *
 * Codes. Every code the encode takes: k >= 1, m >= 0, k + m <= 256. m == 0 or nblocks == 0 returns
 * FEC_OK and touches nothing.
 *
 * Per block. C_b empty: no byte of the block is read or written. Otherwise bytes [0, shard_len) of
 * each of the m parity slots become old parity ^ the sum above, bytes [shard_len, round_up(shard_len,
 * 16)) of each of the m parity slots are written as zeros (whole 16-byte stores, as every output
 * shard), and nothing else is written. Of the data regions only the slots of the columns in C_b are
 * read, over their first round_up(shard_len, 16) bytes, old and new alike; bytes at and past shard_len
 * of any slot never influence bytes [0, shard_len) of the result. old_data and new_data are only
 * read: the call does not copy new over old (as klauspost's Update does not). The parity region
 * must not overlap either data region; this is not checked.
 *
 * klauspost's errors. EncodeIdx's idx out of range (ErrInvShardNum) has no counterpart: a bit at or
 * above k is ignored. Update's "new shard given but old shard nil" cannot arise: every old slot
 * exists, and the mask alone says which columns changed. As with klauspost's EncodeIdx, the parity
 * must start as zeros (over the slots' first round_up(shard_len, 16) bytes) and each column must be
 * added exactly once for the result to be the encode's parity; neither is checked. A full mask on
 * zeroed parity gives byte for byte what fec_rs_encode_batch writes.
 *
 * FEC_DEVICE only: any other `flags` value returns FEC_ERR_INVALID_ARG. There is no host-resident
 * form: it would move the changed shards and the parity both ways over the host link, more than a
 * CPU update touches where the shards already are. Asynchronous on the ctx stream; the calls never
 * touch the sticky word. The layout and alignment rules are the uniform calls', for all three
 * regions with the one shard_stride; the host-side checks run in the uniform order: shard counts,
 * k + m > 256, flags, shard_len (0: FEC_ERR_SHARD_NO_DATA, above 2^30: FEC_ERR_INVALID_ARG),
 * mask_words, the ctx, nblocks == 0 or m == 0 (FEC_OK), null pointers (the mask, the data regions,
 * parity), the layouts (new data or data, parity, old data), the mask's alignment. Batches are cut
 * into launches as the encode cuts them, codes of m > 16 into passes of 16 parity rows, each of
 * which reads the block's masked columns again.
 *
 * Cost. A call moves (c*s + 2*m) shard slots per block for c masked columns (s = 2 for update, 1 for
 * encode-idx) where the encode moves k + m: accumulating a whole block one column at a time moves
 * k*(1 + 2*m). The calls are for callers that hold only some of a block's shards or need the parity
 * one fold after the last shard; they are not a faster encode. */
int fec_rs_update_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                        const uint8_t *old_data, size_t old_block_stride,
                        const uint8_t *new_data, size_t new_block_stride,
                        uint8_t *parity, size_t parity_block_stride,
                        size_t shard_stride, const uint32_t *changed_mask, size_t mask_words,
                        int flags);
int fec_rs_encode_idx_batch(fec_ctx *ctx, int k, int m, size_t shard_len, size_t nblocks,
                            const uint8_t *data, size_t data_block_stride,
                            uint8_t *parity, size_t parity_block_stride,
                            size_t shard_stride, const uint32_t *idx_mask, size_t mask_words,
                            int flags);

/* XOR(k, 1) encode: parity = XOR of the k data shards. */
int fec_xor_encode_batch(fec_ctx *ctx, int k, size_t shard_len, size_t nblocks,
                         const uint8_t *data, size_t data_block_stride,
                         uint8_t *parity, size_t parity_block_stride,
                         size_t shard_stride, int flags);

/* XOR(k, 1) recovery, in place (shard k is the parity): a single missing data shard is the
 * XOR of the other k shards. Two or more missing shards with a data shard among them ->
 * FEC_ERR_TOO_FEW_SHARDS for that block. */
int fec_xor_reconstruct_batch(fec_ctx *ctx, int k, size_t shard_len, size_t nblocks,
                              uint8_t *data, size_t data_block_stride,
                              const uint8_t *parity, size_t parity_block_stride,
                              size_t shard_stride, const uint32_t *present_mask,
                              int32_t *block_status, int flags);

#ifdef __cplusplus
}
#endif
#endif /* FEC_HIP_H */
