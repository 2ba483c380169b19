/* fec_hip_matrix.h — the code matrix of the RS calls: klauspost's default, its WithCauchyMatrix, or
 * rows of the caller's own (its WithCustomMatrix).
 * Part of lib0xfec_hip's C ABI; conventions (return codes, layouts, alignment, stream order, the
 * sticky error word and fec_sync()) are those of fec_hip.h. */
#ifndef FEC_HIP_MATRIX_H
#define FEC_HIP_MATRIX_H

#include "fec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* klauspost New(k, m) with default options: vandermonde(n, k) * inverse(its top k x k). The matrix of
 * fec_rs_matrix and of every ctx until told otherwise. */
#define FEC_MATRIX_VANDERMONDE 0
/* klauspost WithCauchyMatrix: identity on top, M[r][c] = 1 / (r ^ c) for r >= k, field 0x11D. ISA-L's
 * gf_gen_cauchy1_matrix is the same matrix. */
#define FEC_MATRIX_CAUCHY 1

/* The n x k systematic matrix of a kind, n = k + m, row-major into out (n * k bytes). No device is
 * needed. Kind FEC_MATRIX_VANDERMONDE is fec_rs_matrix. An unknown kind or a null out returns
 * FEC_ERR_INVALID_ARG; the shard counts are checked as fec_rs_matrix checks them. */
int fec_rs_matrix_kind(int kind, int k, int m, uint8_t *out);

/* The matrix kind of a ctx. It binds the way klauspost's option binds at New: every RS call made on
 * the ctx afterwards (encode, update, encode-idx, verify, every reconstruct and recover form, the
 * ragged and host-resident forms, the locate family) uses that kind's code for its (k, m). The XOR
 * calls have no matrix and ignore it. A new ctx has kind FEC_MATRIX_VANDERMONDE.
 *
 * Setting the kind is legal between calls without a sync: the ctx keeps the tables of every
 * (kind, k, m) it has used until it is destroyed, and launches already queued keep reading the
 * tables they were given. An unknown kind returns FEC_ERR_INVALID_ARG and leaves the ctx as it was;
 * so does a null ctx (or a null kind pointer). Neither call touches the device. */
int fec_ctx_set_matrix(fec_ctx *ctx, int kind);
int fec_ctx_get_matrix(fec_ctx *ctx, int *kind);

/* klauspost WithCustomMatrix: a code whose parity rows the caller gives. There is nothing to
 * generate, so fec_rs_matrix_kind refuses this kind; fec_ctx_set_matrix accepts it and switches the
 * ctx (back) to the codes registered below. */
#define FEC_MATRIX_CUSTOM 2

/* Register a custom code for (k, m) on the ctx and set the ctx's kind to FEC_MATRIX_CUSTOM.
 * parity_rows is m * k bytes, row-major, klauspost's WithCustomMatrix argument: the code is the
 * identity on top and those rows below, field 0x11D. The shard counts are checked first, as
 * fec_rs_matrix checks them; then a null ctx, null rows or m == 0 returns FEC_ERR_INVALID_ARG. The rows are not
 * validated any further: zeros are legal and so are dependent rows, as in klauspost.
 *
 * Several (k, m) may be registered on one ctx. Registering (k, m) again with other rows makes a new
 * code; launches already queued keep the tables they were given, and every code lives until the ctx
 * is destroyed. Registering rows identical to an earlier registration of (k, m) reuses that code.
 * Like fec_ctx_set_matrix the call is legal between calls without a sync and does not touch the
 * device.
 *
 * Under kind FEC_MATRIX_CUSTOM an RS call for a (k, m) with no registered matrix returns
 * FEC_ERR_NO_MATRIX before any device work. Served: encode, ragged encode, update, encode-idx,
 * verify and ragged verify (fec_rs_verify_ragged_batch, fec_hip_ragged.h) for every k + m <= 256, and
 * for k + m <= FEC_MAX_DECODE_SHARDS reconstruct, recover, their ragged forms, reconstruct-some and
 * ragged reconstruct-some (fec_rs_reconstruct_some_ragged_batch), with the host-resident forms of the
 * calls that have one. The wide
 * reconstruct and recover calls, wide reconstruct-some (each with more than one mask word or a code
 * of more than FEC_MAX_DECODE_SHARDS shards) and the three locate calls are not served under a custom
 * matrix: they return FEC_ERR_NO_MATRIX before any device work.
 *
 * Decoding follows klauspost: the rows of the first k present shards are inverted. A custom code
 * need not be MDS, so k present shards do not guarantee a decode: a block that has enough shards
 * and enough output slots but whose rows are dependent gets status FEC_ERR_SINGULAR, not a byte of
 * it is written, and fec_sync() returns FEC_ERR_SINGULAR if no other failure is pending. With e
 * erased data shards the parity rows used are the first e present ones; the library does not look
 * past them for a solvable set. A caller who knows a better choice steers it by clearing the bits
 * of the parity shards to pass over in the block's present mask. */
int fec_ctx_set_custom_matrix(fec_ctx *ctx, int k, int m, const uint8_t *parity_rows);

#ifdef __cplusplus
}
#endif

#endif /* FEC_HIP_MATRIX_H */
