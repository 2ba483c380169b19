// rs_matrix.hpp — host-side construction of the systematic Reed-Solomon matrix.
//
// Produces the same matrix as github.com/klauspost/reedsolomon v1.12.4 `New(k, m)` with
// default options (reference call site internal/fec/reed_solomon.go:16, manager.go:60,83):
//   vandermonde(n, k)[r][c] = r^c   (galExp semantics: 0^0 = 1)
//   M = vandermonde * inverse(top k x k of vandermonde)
// Any k rows of M are linearly independent (row-equivalent to a Vandermonde matrix with
// distinct evaluation points), which the reconstruct plan relies on.
#pragma once

#include <stdint.h>

#include <vector>

#include "gf256.h"

namespace rs {

// Invert an n x n matrix in place (row-major). Returns false if singular.
inline bool invert(int n, uint8_t* m) {
    const int w = 2 * n;
    std::vector<uint8_t> a((size_t)n * w, 0);
    for (int r = 0; r < n; ++r) {
        for (int c = 0; c < n; ++c) a[(size_t)r * w + c] = m[(size_t)r * n + c];
        a[(size_t)r * w + n + r] = 1;
    }
    for (int col = 0; col < n; ++col) {
        int piv = -1;
        for (int r = col; r < n; ++r)
            if (a[(size_t)r * w + col]) { piv = r; break; }
        if (piv < 0) return false;
        if (piv != col)
            for (int c = 0; c < w; ++c) std::swap(a[(size_t)piv * w + c], a[(size_t)col * w + c]);
        const uint8_t s = gf::inv(a[(size_t)col * w + col]);
        for (int c = 0; c < w; ++c) a[(size_t)col * w + c] = gf::mul(s, a[(size_t)col * w + c]);
        for (int r = 0; r < n; ++r) {
            if (r == col) continue;
            const uint8_t f = a[(size_t)r * w + col];
            if (!f) continue;
            for (int c = 0; c < w; ++c) a[(size_t)r * w + c] ^= gf::mul(f, a[(size_t)col * w + c]);
        }
    }
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) m[(size_t)r * n + c] = a[(size_t)r * w + n + c];
    return true;
}

// n x k systematic encoding matrix, row-major. Empty on failure.
inline std::vector<uint8_t> build_matrix(int k, int n) {
    std::vector<uint8_t> out;
    if (k <= 0 || n < k || n > 256) return out;
    std::vector<uint8_t> vm((size_t)n * k), top((size_t)k * k);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < k; ++c) vm[(size_t)r * k + c] = gf::exp_pow((uint8_t)r, c);
    for (size_t i = 0; i < top.size(); ++i) top[i] = vm[i];
    if (!invert(k, top.data())) return out;
    out.assign((size_t)n * k, 0);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < k; ++c) {
            uint8_t acc = 0;
            for (int t = 0; t < k; ++t) acc ^= gf::mul(vm[(size_t)r * k + t], top[(size_t)t * k + c]);
            out[(size_t)r * k + c] = acc;
        }
    return out;
}

// The matrix kinds of fec_hip_matrix.h (FEC_MATRIX_*).
constexpr int kMatrixVandermonde = 0, kMatrixCauchy = 1, kMatrixKinds = 2;

// klauspost WithCauchyMatrix (ISA-L gf_gen_cauchy1_matrix over the same field): identity on top,
// M[r][c] = 1 / (r ^ c) for r >= k. Every square submatrix of a Cauchy matrix is invertible, so any
// k rows of M are independent. Empty on failure.
inline std::vector<uint8_t> build_cauchy_matrix(int k, int n) {
    std::vector<uint8_t> out;
    if (k <= 0 || n < k || n > 256) return out;
    out.assign((size_t)n * k, 0);
    for (int r = 0; r < k; ++r) out[(size_t)r * k + r] = 1;
    for (int r = k; r < n; ++r)
        for (int c = 0; c < k; ++c) out[(size_t)r * k + c] = gf::inv((uint8_t)(r ^ c));
    return out;
}

// The n x k systematic matrix of a kind; empty on failure (an unknown kind among them).
inline std::vector<uint8_t> build_matrix_kind(int kind, int k, int n) {
    if (kind == kMatrixVandermonde) return build_matrix(k, n);
    if (kind == kMatrixCauchy) return build_cauchy_matrix(k, n);
    return {};
}

// Both kinds are generalized Reed-Solomon codes on the points 0 .. n-1: shard r of a consistent block
// is v_r p(r) for one polynomial p of degree < k. The default code has v = 1. For the Cauchy code,
// interpolating x_c / v_c at the data points and evaluating at r >= k gives
// prod_{t<k} (r ^ t) * sum_c x_c / (r ^ c), so v_r = 1 / prod_{c<k, c != r} (r ^ c) for every r.
// Returns log v_r mod 255 for r < n: all a decode plan or a locate table needs beyond the points.
inline std::vector<uint8_t> grs_logv(int kind, int k, int n) {
    std::vector<uint8_t> lv((size_t)n, 0);
    if (kind != kMatrixCauchy) return lv;
    for (int r = 0; r < n; ++r) {
        unsigned s = 0;
        for (int c = 0; c < k; ++c)
            if (c != r) s += gf::kTables.log[r ^ c];
        lv[(size_t)r] = (uint8_t)((255u - s % 255u) % 255u);
    }
    return lv;
}

}  // namespace rs
