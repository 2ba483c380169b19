/* fec_hip_matrix.h — the code matrix of the RS calls: klauspost's default, or its WithCauchyMatrix.
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

#ifdef __cplusplus
}
#endif

#endif /* FEC_HIP_MATRIX_H */
