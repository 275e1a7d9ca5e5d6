// logprob.h — token log-likelihoods of R rows of fp32 logits (lmi_token_logprobs): the scoring tail of forward(labels=) /
// LeopardEngine.score.  For row r (source row rows[r], or r) with the vocabulary in columns [0, vocab):
//   lse[r]     = log sum_i exp(logit_i)                     (i < vocab; columns >= vocab — the head's padding — are never read)
//   logprob[r] = logit[targets[r]] - lse[r]                 (NaN when targets[r] is outside [0, vocab))
//   argmax[r]  = the id of the largest logit, lowest index on ties (decode_advance_kernel's rule; NaN never wins; 0 for an all-NaN row)
// How: one 512-thread workgroup per row, ONE pass over the row with 16-byte loads, four in flight per lane (sample_for_row's scan).
// Each lane keeps an online (max m, sum s of exp(x - m)) pair and its best (value, index); the pairs are merged across the wave by a
// fixed butterfly, then across the eight waves by thread 0 in wave order.  No atomics anywhere: the results are bit-identical from run
// to run.  No allocation and no host synchronisation: the launch is graph-capturable.  The scan and the merges are device functions
// (lse_scan_lane / lse_wave_merge / lse_block_finish) that decode_logprobs_kernel (decode_logprob.h) shares, so both give a row the same lse bits.
#pragma once
#include "elementwise.h"

namespace lmi {

struct TokenLogprobArgs {
    const float* logits;          // [., ld] fp32, rows 16-byte aligned
    const int64_t* rows;          // [R] nullable: logits row of output r (null: row r)
    const int64_t* targets;       // [R]
    int vocab, ld;
    float* logprob;               // [R]
    float* lse;                   // [R]
    int64_t* argmax;              // [R]
};

constexpr int kLogprobThreads = 512;
constexpr float kLogprobLog2e = 1.4426950408889634f;

// (m, s) <- (m, s) (+) (m2, s2), where s carries exp(. - m).  An empty side is (-inf, 0).
LMI_DEV void lse_merge(float& m, float& s, float m2, float s2) {
    if (m2 > m) {
        s = (m > -INFINITY ? s * exp2f((m - m2) * kLogprobLog2e) : 0.f) + s2;
        m = m2;
    } else if (m2 > -INFINITY) {
        s += s2 * exp2f((m2 - m) * kLogprobLog2e);
    }
}

// The row scan of both logprob kernels (token_logprobs_kernel here, decode_logprobs_kernel in decode_logprob.h): the lane's online
// (m, s) over its share of row[0 .. V), 16-byte loads, four in flight; each(x, i) sees every element the lane visits, indices ascending.
template <typename F>
LMI_DEV void lse_scan_lane(const float* row, int V, float& m, float& s, F&& each) {
    const int tid = threadIdx.x, nt = (int)blockDim.x, v4 = V >> 2;
    auto take4 = [&](const f32x4 q, int i) {
        const float cm = fmaxf(fmaxf(q[0], q[1]), fmaxf(q[2], q[3]));
        if (cm > m) {
            s = m > -INFINITY ? s * exp2f((m - cm) * kLogprobLog2e) : 0.f;
            m = cm;
        }
        if (m > -INFINITY) {
#pragma unroll
            for (int e = 0; e < 4; ++e) s += exp2f((q[e] - m) * kLogprobLog2e);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) each(q[e], i + e);
    };
    for (int i0 = tid; i0 < v4; i0 += 4 * nt) {
        f32x4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * nt;
            q[u] = i < v4 ? *(const f32x4*)(row + 4 * (long)i) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * nt;
            if (i < v4) take4(q[u], 4 * i);
        }
    }
    for (int i = 4 * v4 + tid; i < V; i += nt) {                      // vocab % 4 tail (above every vector index of the lane)
        const float x = row[i];
        lse_merge(m, s, x, x > -INFINITY ? 1.f : 0.f);
        each(x, i);
    }
}

// the wave's 64 pairs into every lane, by a fixed butterfly
LMI_DEV void lse_wave_merge(float& m, float& s) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const float om = shfl_xor(m, k), os = shfl_xor(s, k);
        lse_merge(m, s, om, os);
    }
}

// thread 0, after the waves' lane-0 pairs went to red_m / red_s and a barrier: the waves merged in wave order -> the row's lse
LMI_DEV float lse_block_finish(float m, float s, const float* red_m, const float* red_s, int nw) {
    for (int w = 1; w < nw; ++w) lse_merge(m, s, red_m[w], red_s[w]);
    return m + logf(s);
}

__global__ void __launch_bounds__(kLogprobThreads) token_logprobs_kernel(TokenLogprobArgs a) {
    __shared__ float red_m[kLogprobThreads / 64], red_s[kLogprobThreads / 64], red_v[kLogprobThreads / 64];
    __shared__ int red_i[kLogprobThreads / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
    const float* row = a.logits + (a.rows ? a.rows[r] : (int64_t)r) * (int64_t)a.ld;
    const int V = a.vocab;
    float m = -INFINITY, s = 0.f, bv = -INFINITY;
    int bi = 0x7fffffff;
    // a lane visits its indices in increasing order: a strict '>' keeps the lowest index of a tie
    lse_scan_lane(row, V, m, s, [&](float x, int i) {
        if (x > bv) { bv = x; bi = i; }
    });
    lse_wave_merge(m, s);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const float ov = shfl_xor(bv, k);
        const int oi = shfl_xor(bi, k);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_m[wave] = m; red_s[wave] = s; red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nw; ++w)
            if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi)) { bv = red_v[w]; bi = red_i[w]; }
        const float l = lse_block_finish(m, s, red_m, red_s, nw);
        const int64_t t = a.targets[r];
        a.lse[r] = l;
        a.logprob[r] = (t >= 0 && t < (int64_t)V) ? row[t] - l : NAN;
        a.argmax[r] = bi == 0x7fffffff ? 0 : bi;
    }
}

}  // namespace lmi
