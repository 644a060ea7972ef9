// Internal header of the pointwise-conv family: the kernel families that the routes of pwgemm.hip (forward, data gradient) and pwwgrad.hip (weight
// gradient) choose between (gate.hip, pwthin.hip, pwwide.hip, pwwgs.hip, pwntv1.hip), the few things those two units and pwbnbwd.hip share, and the
// finalize of the fused expand-unit backward (pwbnbwd.hip) that exdw.hip, gate.hip and stemdw.hip use too.  The other sources do not see these.
// Not part of the C ABI (include/mnyolo.h).
#pragma once
#include "common.h"

namespace mny {

// thin pointwise conv forward / plain data gradient, bf16 storage, a wave per 16 pixels on the matrix cores (gate.hip)
bool pwt_ok(int64_t M, int K, int N, int in_act, bool has_bias);
int pwt_parts(int64_t M);
int pwt_launch(const void* x, const float* xs, const float* xb, int xact, const void* w, const void* addend, void* y, float* stats, int64_t M, int K, int N,
               hipStream_t st, const void* rY = nullptr, const float* r_scale = nullptr, const float* r_shift = nullptr, const float* r_mean = nullptr,
               const float* r_invstd = nullptr, int r_act = 0);      // rY != NULL: the data-gradient + BN-backward-sums form (stats = the partial rows)

// thin expand unit backward on bf16 storage, wave form (gate.hip pwe_sums_kernel / pwe_dgrad_kernel); pw_bnbwd_finalize_launch: pwbnbwd.hip
bool pwe_ok(int64_t M, int K, int N);
size_t pwe_ws_floats(int64_t M, int K, int N);
int pwe_launch(const void* g, const void* y, const float* scale, const float* shift, int act, const float* mean, const float* invstd, const float* gamma,
               const void* x, const float* in_scale, const float* in_shift, int in_act, const float* w, const void* addend, void* dx, float* dw,
               float* dgamma, float* dbeta, float* ws, int64_t M, int K, int Nc, hipStream_t st);

// short-reduction pointwise conv on the vector ALU (pwthin.hip); the routes of pwgemm.hip send K = 8/16/24/32 problems here
bool pw_thin_ok(int bf, int red, int64_t M, int K, int N);
int pw_thin_parts(int64_t M, int K, int N, int red);
int pw_thin_launch(int bf, const void* A, const float* in_scale, const float* in_shift, int in_act, const void* W, const float* bias,
                   const void* addend, void* C, float* stats, int64_t M, int K, int N, int red, const void* rY, const float* r_scale,
                   const float* r_shift, const float* r_mean, const float* r_invstd, int r_act, hipStream_t st);

// short reduction feeding a wide output (K = 52..96, N >= K): barrier-free matrix-core kernel (pwwide.hip); fp32 storage only
bool pw_wide_ok(int64_t M, int K, int N, bool red);       // red: the data-gradient + BN-backward-sums form
int pw_wide_parts(int64_t M, int K, int N, bool red);       // partial rows of the whole 32-row tiles
int pw_wide_launch(const float* A, const float* in_scale, const float* in_shift, int in_act, const float* W, float* C, float* stats,
                   int64_t M, int K, int N, const float* rY, const float* r_scale, const float* r_shift, const float* r_mean,
                   const float* r_invstd, int r_act, const float* addend, hipStream_t st);

// mny_pw_lr_fix on the barrier-free kernel (K = 64 / 96, whole 32-row tiles): dx = (in_scale o x + in_shift) Q + bias + addend, + the sums
bool pw_wide_fix_ok(int64_t M, int K);
int pw_wide_fix_parts(int64_t M, int K);
int pw_wide_fix_launch(const float* A, const float* in_scale, const float* in_shift, const float* Q, const float* bias, const float* addend, float* C,
                       float* stats, int64_t M, int K, const float* rY, const float* r_scale, const float* r_shift, const float* r_mean,
                       const float* r_invstd, int r_act, hipStream_t st);

// register-staged NT kernel (pwntv1.hip): any K, either storage type (bf: the operands are bf16_t); the MNY_ROUTE_TILE_V1 family of pwgemm.hip
int pw_v1_parts(int64_t M, int K, int N);
int pw_v1_launch(int bf, const void* x, const float* in_scale, const float* in_shift, int in_act, const void* w, const float* bias, const void* addend,
                 void* y, float* stats, int64_t M, int K, int N, hipStream_t st);

// weight gradient with one narrow side (64 / 96 channels): barrier-free stream kernel (pwwgs.hip); fp32 storage, no bias gradient
bool pw_wgs_ok(int64_t M, int K, int N);
int pw_wgs_splits(int64_t M, int K, int N);
int pw_wgs_launch(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* dy, float* partial,
                  int64_t M, int K, int N, hipStream_t st);

// fp32 GEMMs whose matrix-core time exceeds their HBM time take the six-product bf16 form (MNY_X6=0: never, =1: always, for A/B runs): one rule for
// the routes of pwgemm.hip and the weight gradient's (pwwgrad.hip)
inline int nt_x6(int64_t M, int K, int N) {
    const int env = sw(SW_X6);
    if (env >= 0) return env != 0;
    const double ai = 2.0 * K * N / (4.0 * (K + N));            // FLOP per byte of the A and C rows
    return ai >= 20.0;                                          // 157 TFLOP/s / 8 TB/s
}

// the seams between pwgemm.hip and pwwgrad.hip: a weight-gradient call is this thread's last pointwise-conv call too (mny_pw_last_route reads one
// variable, defined in pwgemm.hip), and mny_pw_route(op = 2) reports the family pw_wgrad_route gives the plain call (no view, no bias gradient)
void pw_set_last_route(int family);
int pw_wgrad_family(int bf, int64_t M, int K, int N);

// partial rows [nparts][n] -> out[n] in fp64, fixed order: the launch of reduce_parts_kernel (compiled once, in pwwgrad.hip) for pwbnbwd.hip;
// the caller checks the launch
void reduce_parts_launch(const float* parts, int nparts, int64_t n, float* out, hipStream_t st);

// fused BN-backward of a thin expand unit (pwbnbwd.hip): partial row layout  P1[N*K] | Gram[K*K] | s1[N] | s2[N] | s3[K]  and its fp64 finalize
// (-> dW, dgamma, dbeta and the data-gradient operands B1[K][N] = ca o W^T, Q[K][K] = W^T diag(cb) W, bias[K] = cc . W)
__host__ __device__ inline int64_t bnw_stride(int N, int K) { return (int64_t)N * K + (int64_t)K * K + 2 * N + K; }
int pw_bnbwd_finalize_launch(const float* partials, int nparts, float* red, const float* w, const float* gamma, const float* mean,
                             const float* invstd, int64_t M, int Nc, int K, float* dw, float* dgamma, float* dbeta, float* B1, float* Q,
                             float* bias, hipStream_t st);

}  // namespace mny
