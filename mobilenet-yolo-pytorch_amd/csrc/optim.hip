// Fused multi-tensor AdamW: one launch updates every parameter tensor of the model.
//
// replaces `optim.AdamW(model.parameters(), lr, weight_decay)` + `optimizer.step()` (train.py:134,283): PyTorch's update
//     p  <- p * (1 - lr*wd)                                   (decoupled weight decay)
//     m  <- m + (1-b1)*(g - m) ;  v <- b2*v + (1-b2)*g*g
//     p  <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// (amsgrad = False, maximize = False; the caller passes the two bias corrections, so `step` stays on the host).
// HBM-bound: 4 reads + 3 writes of 4 B per parameter (4.9 M parameters -> 138 MB, ~30 us), against 202 small launches upstream.
// The chunk table lives in device memory and is built once per model (parameter / gradient-arena / state pointers are stable).
// Further down, on the same chunk rows: fused SGD with momentum, the weight EMA and the shadow <-> weights swap.
#include "common.h"

namespace mny {

// omb1 / omb2 = 1 - beta, rounded from DOUBLE like torch's python-side `1 - beta2` (1.f - 0.999f is off by 4.7e-5 relative)
// every scalar is derived on the host in DOUBLE (as torch derives them from python floats) and rounded once
__global__ __launch_bounds__(256) void adamw_kernel(const mny_adamw_chunk* __restrict__ table, int nchunks, float decay, float step,
                                                   float omb1, float beta2, float omb2, float rs2, float eps) {
    const int ci = blockIdx.x;
    if (ci >= nchunks) return;
    const mny_adamw_chunk ch = table[ci];
    float* __restrict__ p = ch.p;
    const float* __restrict__ g = ch.g;
    float* __restrict__ m = ch.m;
    float* __restrict__ v = ch.v;
    auto upd = [&](float pv, float gv, float& mv, float& vv) {
        pv *= decay;
        mv = fmaf(omb1, gv - mv, mv);                            // torch's exp_avg.lerp_(grad, 1 - beta1)
        vv = beta2 * vv + omb2 * gv * gv;
        return pv - step * mv / (sqrtf(vv) * rs2 + eps);
    };
    const int n4 = ch.vec4 ? ch.n / 4 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 pv = ld4(p + 4 * i), mv = ld4(m + 4 * i), vv = ld4(v + 4 * i);
        const float4 gv = ld4(g + 4 * i);
        pv.x = upd(pv.x, gv.x, mv.x, vv.x); pv.y = upd(pv.y, gv.y, mv.y, vv.y);
        pv.z = upd(pv.z, gv.z, mv.z, vv.z); pv.w = upd(pv.w, gv.w, mv.w, vv.w);
        st4(p + 4 * i, pv); st4(m + 4 * i, mv); st4(v + 4 * i, vv);
    }
    for (int i = n4 * 4 + threadIdx.x; i < ch.n; i += 256) {
        float mv = m[i], vv = v[i];
        p[i] = upd(p[i], g[i], mv, vv);
        m[i] = mv; v[i] = vv;
    }
}

// ---- fused gradient clipping (mny_grad_clip): two streaming passes over the gradient segments, HBM-bound ----
// One workgroup per MNY_CLIP_BLOCK floats of a segment.  The block's first element sits (block index) * 8192 floats behind the
// segment's, so every block of a segment has the segment's alignment: up to 3 scalar head elements reach the 16-byte boundary,
// float4 loads / stores cover the body, up to 3 scalars the tail.
struct clip_span {
    float* g;          // first element of this workgroup's block
    int cnt, head, n4; // elements, scalar head elements, float4 of the body
};

__device__ __forceinline__ clip_span clip_find(const mny_clip_seg* __restrict__ segs, int nsegs, int b) {
    int lo = 0, hi = nsegs - 1;                                  // the last segment whose block0 <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].block0 <= b) lo = mid; else hi = mid - 1;
    }
    const mny_clip_seg sg = segs[lo];
    const int64_t off = (int64_t)(b - sg.block0) * MNY_CLIP_BLOCK;
    int64_t left = sg.n - off;                                   // (a table whose block0 column disagrees with the lengths yields empty blocks, never an access outside a segment)
    if (b < sg.block0 || left < 0) left = 0;
    clip_span sp;
    sp.cnt = (int)(left < MNY_CLIP_BLOCK ? left : MNY_CLIP_BLOCK);
    sp.g = sg.g + off;
    const int mis = (int)((reinterpret_cast<uintptr_t>(sp.g) >> 2) & 3);
    const int head = (4 - mis) & 3;
    sp.head = head < sp.cnt ? head : sp.cnt;
    sp.n4 = (sp.cnt - sp.head) >> 2;
    return sp;
}

// fixed-order fp64 tree over the workgroup's 256 values; every thread returns the total
__device__ __forceinline__ double clip_block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void clip_sumsq_kernel(const mny_clip_seg* __restrict__ segs, int nsegs, double* __restrict__ ws) {
    __shared__ double sh[256];
    const clip_span sp = clip_find(segs, nsegs, blockIdx.x);
    const int t = threadIdx.x;
    const float* __restrict__ body = sp.g + sp.head;
    float acc = 0.f;                                             // <= 8 float4 + 1 head + 1 tail scalar = MNY_CLIP_TERMS squares
    for (int i = t; i < sp.n4; i += 256) {
        const float4 v = ld4(body + 4 * i);
        acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
    }
    if (t < sp.head) acc = fmaf(sp.g[t], sp.g[t], acc);
    const int ts = sp.head + 4 * sp.n4;
    if (t < sp.cnt - ts) acc = fmaf(sp.g[ts + t], sp.g[ts + t], acc);
    const double tot = clip_block_sum((double)acc, sh);
    if (t == 0) ws[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void clip_scale_kernel(const mny_clip_seg* __restrict__ segs, int nsegs, const double* __restrict__ ws, int nblocks,
                                                        float max_norm, float* __restrict__ out) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < nblocks; i += 256) s += ws[i];           // the same order in every workgroup: they all form the same coefficient
    const float tn = (float)sqrt(clip_block_sum(s, sh));
    float coef = max_norm / (tn + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;                              // torch.clamp(max=1): NaN stays NaN
    if (blockIdx.x == 0 && t == 0) { out[0] = tn; out[1] = coef; }
    if (coef == 1.f) return;                                     // nothing to scale (g * 1 is g)
    const clip_span sp = clip_find(segs, nsegs, blockIdx.x);
    float* body = sp.g + sp.head;
    for (int i = t; i < sp.n4; i += 256) {
        float4 v = ld4(body + 4 * i);
        v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
        st4(body + 4 * i, v);
    }
    if (t < sp.head) sp.g[t] *= coef;
    const int ts = sp.head + 4 * sp.n4;
    if (t < sp.cnt - ts) sp.g[ts + t] *= coef;
}

// ---- fused multi-tensor SGD (mny_sgd_step), weight EMA (mny_ema_update) and the shadow swap (mny_swap_chunks) ----
// The same chunk rows and launch shape as adamw_kernel: one workgroup per chunk, float4 body, scalar tail.  HBM-bound streams:
// SGD with momentum 3 reads + 2 writes of 4 B per element, the EMA 2 reads + 1 write, the swap 2 + 2.
// Every product-sum is written as the fmaf torch's own kernels contract to (`add(other, alpha)` is one a + alpha*b):
//     d = g + wd*p ; buf = (mu*buf) + (1-damp)*d ; d = d + mu*buf ; p = p + (-lr)*d
// WD: weight_decay != 0.  MOM: 0 = no momentum (ch.m is NULL and never touched), 1 = first step (buf = d, ch.m written only), 2 = running.
template <bool WD, int MOM, bool NEST>
__global__ __launch_bounds__(256) void sgd_kernel(const mny_adamw_chunk* __restrict__ table, int nchunks, float neg_lr, float mu, float omd, float wd) {
    const int ci = blockIdx.x;
    if (ci >= nchunks) return;
    const mny_adamw_chunk ch = table[ci];
    float* __restrict__ p = ch.p;
    const float* __restrict__ g = ch.g;
    float* __restrict__ m = ch.m;
    auto upd = [&](float pv, float gv, float& mv) {
        float d = WD ? fmaf(wd, pv, gv) : gv;
        if (MOM == 1) mv = d;
        if (MOM == 2) mv = fmaf(omd, d, mu * mv);
        if (MOM != 0) d = NEST ? fmaf(mu, mv, d) : mv;
        return fmaf(neg_lr, d, pv);
    };
    const int n4 = ch.vec4 ? ch.n / 4 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 pv = ld4(p + 4 * i), mv = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 gv = ld4(g + 4 * i);
        if (MOM == 2) mv = ld4(m + 4 * i);
        pv.x = upd(pv.x, gv.x, mv.x); pv.y = upd(pv.y, gv.y, mv.y);
        pv.z = upd(pv.z, gv.z, mv.z); pv.w = upd(pv.w, gv.w, mv.w);
        st4(p + 4 * i, pv);
        if (MOM != 0) st4(m + 4 * i, mv);
    }
    for (int i = n4 * 4 + threadIdx.x; i < ch.n; i += 256) {
        float mv = MOM == 2 ? m[i] : 0.f;
        p[i] = upd(p[i], g[i], mv);
        if (MOM != 0) m[i] = mv;
    }
}

// m <- m + (1 - decay) * (p - m): torch.lerp for a weight below 0.5, one fmaf.  p is read only.
__global__ __launch_bounds__(256) void ema_kernel(const mny_adamw_chunk* __restrict__ table, int nchunks, float omd) {
    const int ci = blockIdx.x;
    if (ci >= nchunks) return;
    const mny_adamw_chunk ch = table[ci];
    const float* __restrict__ p = ch.p;
    float* __restrict__ m = ch.m;
    const int n4 = ch.vec4 ? ch.n / 4 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 pv = ld4(p + 4 * i);
        float4 mv = ld4(m + 4 * i);
        mv.x = fmaf(omd, pv.x - mv.x, mv.x); mv.y = fmaf(omd, pv.y - mv.y, mv.y);
        mv.z = fmaf(omd, pv.z - mv.z, mv.z); mv.w = fmaf(omd, pv.w - mv.w, mv.w);
        st4(m + 4 * i, mv);
    }
    for (int i = n4 * 4 + threadIdx.x; i < ch.n; i += 256) {
        const float mv = m[i];
        m[i] = fmaf(omd, p[i] - mv, mv);
    }
}

// p[0..n) <-> m[0..n): every element is read and written by one thread, so the exchange is exact and two calls are the identity
__global__ __launch_bounds__(256) void swap_kernel(const mny_adamw_chunk* __restrict__ table, int nchunks) {
    const int ci = blockIdx.x;
    if (ci >= nchunks) return;
    const mny_adamw_chunk ch = table[ci];
    float* __restrict__ p = ch.p;
    float* __restrict__ m = ch.m;
    const int n4 = ch.vec4 ? ch.n / 4 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 pv = ld4(p + 4 * i), mv = ld4(m + 4 * i);
        st4(p + 4 * i, mv); st4(m + 4 * i, pv);
    }
    for (int i = n4 * 4 + threadIdx.x; i < ch.n; i += 256) {
        const float pv = p[i];
        p[i] = m[i];
        m[i] = pv;
    }
}

template <bool WD, int MOM, bool NEST>
static int sgd_launch(const mny_adamw_chunk* table, int nchunks, float neg_lr, float mu, float omd, float wd, hipStream_t stream) {
    hipLaunchKernelGGL((sgd_kernel<WD, MOM, NEST>), dim3(nchunks), dim3(256), 0, stream, table, nchunks, neg_lr, mu, omd, wd);
    return check_launch("sgd_kernel");
}

template <bool WD>
static int sgd_pick(int mom, bool nest, const mny_adamw_chunk* table, int nchunks, float neg_lr, float mu, float omd, float wd, hipStream_t stream) {
    if (mom == 0) return sgd_launch<WD, 0, false>(table, nchunks, neg_lr, mu, omd, wd, stream);
    if (mom == 1) return nest ? sgd_launch<WD, 1, true>(table, nchunks, neg_lr, mu, omd, wd, stream)
                              : sgd_launch<WD, 1, false>(table, nchunks, neg_lr, mu, omd, wd, stream);
    return nest ? sgd_launch<WD, 2, true>(table, nchunks, neg_lr, mu, omd, wd, stream)
                : sgd_launch<WD, 2, false>(table, nchunks, neg_lr, mu, omd, wd, stream);
}

}  // namespace mny

using namespace mny;

extern "C" int mny_adamw_step(const mny_adamw_chunk* table_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                              double weight_decay, int64_t step, void* stream) {
    MNY_REQUIRE(table_dev && nchunks > 0 && step > 0, "adamw_step: bad arguments");
    MNY_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adamw_step: betas must be in [0,1)");
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    hipLaunchKernelGGL(adamw_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev, nchunks, (float)(1.0 - lr * weight_decay),
                       (float)(lr / bc1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(1.0 / sqrt(bc2)), (float)eps);
    return check_launch("adamw_kernel");
}

extern "C" int mny_grad_clip_parts(int64_t n) {
    MNY_REQUIRE(n >= 0 && n / MNY_CLIP_BLOCK < (1 << 30), "grad_clip_parts: bad length");
    return (int)((n + MNY_CLIP_BLOCK - 1) / MNY_CLIP_BLOCK);
}

extern "C" int mny_grad_clip(const mny_clip_seg* segs_dev, int nsegs, int nblocks, double max_norm, double* ws, float* out, void* stream) {
    MNY_REQUIRE(segs_dev && ws && out, "grad_clip: null pointer");
    MNY_REQUIRE(nsegs > 0 && nblocks > 0, "grad_clip: empty segment table");
    MNY_REQUIRE(max_norm >= 0.0, "grad_clip: max_norm must be >= 0");          // (a NaN max_norm fails this too)
    hipLaunchKernelGGL(clip_sumsq_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, segs_dev, nsegs, ws);
    if (int rc = check_launch("clip_sumsq_kernel")) return rc;
    hipLaunchKernelGGL(clip_scale_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, segs_dev, nsegs, ws, nblocks, (float)max_norm, out);
    return check_launch("clip_scale_kernel");
}

extern "C" int mny_sgd_step(const mny_adamw_chunk* table_dev, int nchunks, double lr, double momentum, double dampening, double weight_decay,
                            int nesterov, int first, void* stream) {
    MNY_REQUIRE(table_dev && nchunks > 0, "sgd_step: bad arguments");
    MNY_REQUIRE(lr >= 0.0 && momentum >= 0.0 && weight_decay >= 0.0, "sgd_step: lr, momentum and weight_decay must be >= 0");      // (NaN fails too)
    MNY_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "sgd_step: nesterov momentum requires a momentum and zero dampening");
    const int mom = momentum == 0.0 ? 0 : (first ? 1 : 2);
    const float neg_lr = (float)-lr, mu = (float)momentum, omd = (float)(1.0 - dampening), wd = (float)weight_decay;
    return weight_decay != 0.0 ? sgd_pick<true>(mom, nesterov != 0, table_dev, nchunks, neg_lr, mu, omd, wd, (hipStream_t)stream)
                               : sgd_pick<false>(mom, nesterov != 0, table_dev, nchunks, neg_lr, mu, omd, wd, (hipStream_t)stream);
}

extern "C" int mny_ema_update(const mny_adamw_chunk* table_dev, int nchunks, double decay, void* stream) {
    MNY_REQUIRE(table_dev && nchunks > 0, "ema_update: bad arguments");
    MNY_REQUIRE(decay >= 0.0 && decay <= 1.0, "ema_update: decay must be in [0,1]");                                                 // (NaN fails too)
    hipLaunchKernelGGL(ema_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev, nchunks, (float)(1.0 - decay));
    return check_launch("ema_kernel");
}

extern "C" int mny_swap_chunks(const mny_adamw_chunk* table_dev, int nchunks, void* stream) {
    MNY_REQUIRE(table_dev && nchunks > 0, "swap_chunks: bad arguments");
    hipLaunchKernelGGL(swap_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, table_dev, nchunks);
    return check_launch("swap_kernel");
}
