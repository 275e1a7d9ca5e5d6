// decode_logprob.h — log-probabilities of the token a decode step just chose, and of the row's top-k alternatives
// (lmi_decode_logprobs): the launch that follows decode_advance_kernel / decode_sample_kernel in the steps captured for
// generate(logprobs=k).  For sequence b, over the RAW logits row (no temperature, no suppress list), columns [0, vocab):
//   lse            = log sum_i exp(logit_i)                  — token_logprobs_kernel's scan and merges (logprob.h): the same bits
//   lp             = logit[tok[b]] - lse                     (NaN when tok[b] is outside [0, vocab))
//   top_id[j], top_lp[j] (j < top_k) = the j-th entry of the row ordered by value descending, id ascending, and its logit - lse;
//                    NaN entries never enter; with fewer than top_k non-NaN entries the rest are -1 / -inf; entries j >= top_k are not written
// all three written to ring slot (hist_pos[b] - 1) mod ring_len (the choice kernel has already advanced the counter; null hist_pos: slot 0).
// How: one 512-thread workgroup per sequence and ONE pass over the row whatever top_k is.  While it scans, a lane keeps the 8 best
// (value, id) pairs it has seen, sorted, in registers: a new element is compared with the lane's 8th and only then sifted in.  The order
// "value descending, id ascending" is a strict total order over a row's entries, so the best 8 of a union of lists is ONE set whatever
// way the lists are merged; the merge is nevertheless fixed — the lse butterfly's lane pairs (xor 32, 16, .. 1), then thread 0 over the
// eight waves in wave order — so a row's result does not depend on B, on its place in the batch or on the run.  No atomics, no allocation,
// no host synchronisation: capturable.
#pragma once
#include "logprob.h"

namespace lmi {

constexpr int kMaxTopLogprobs = 8;

struct DecodeLogprobArgs {
    const float* logits;          // [B, ld] fp32, rows 16-byte aligned
    const int64_t* tok;           // [B] the tokens just chosen
    const int* hist_pos;          // [B] nullable
    int vocab, ld, ring_len, top_k, B;
    float* lp;                    // [ring_len, B]
    int* top_id;                  // [ring_len, B, 8]
    float* top_lp;                // [ring_len, B, 8]
};

// (v, i) comes before (w, j) in the order value descending, id ascending; false whenever v is NaN.  An empty slot is (-inf, INT_MAX):
// after every real entry, a real -inf included.
LMI_DEV bool top_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

struct TopList {
    float v[kMaxTopLogprobs];
    int i[kMaxTopLogprobs];
    LMI_DEV void clear() {
#pragma unroll
        for (int j = 0; j < kMaxTopLogprobs; ++j) { v[j] = -INFINITY; i[j] = 0x7fffffff; }
    }
    // sift (x, id) into the sorted list; the displaced entries move down, the last one falls out (fully unrolled: registers only)
    LMI_DEV void insert(float x, int id) {
#pragma unroll
        for (int j = 0; j < kMaxTopLogprobs; ++j) {
            const bool b = top_before(x, id, v[j], i[j]);
            const float tv = v[j];
            const int ti = i[j];
            v[j] = b ? x : tv; i[j] = b ? id : ti;
            x = b ? tv : x; id = b ? ti : id;
        }
    }
    LMI_DEV void offer(float x, int id) {
        if (top_before(x, id, v[kMaxTopLogprobs - 1], i[kMaxTopLogprobs - 1])) insert(x, id);
    }
};

__global__ void __launch_bounds__(kLogprobThreads) decode_logprobs_kernel(DecodeLogprobArgs a) {
    constexpr int NW = kLogprobThreads / 64, K = kMaxTopLogprobs;
    __shared__ float red_m[NW], red_s[NW], red_v[NW * K];
    __shared__ int red_i[NW * K];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
    const float* row = a.logits + (int64_t)b * (int64_t)a.ld;
    const int V = a.vocab;
    const bool want_top = a.top_k > 0;
    float m = -INFINITY, s = 0.f;
    TopList top;
    top.clear();
    lse_scan_lane(row, V, m, s, [&](float x, int i) {
        if (want_top) top.offer(x, i);
    });
    lse_wave_merge(m, s);
    if (want_top) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
            float ov[K];
            int oi[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { ov[j] = shfl_xor(top.v[j], k); oi[j] = shfl_xor(top.i[j], k); }
#pragma unroll
            for (int j = 0; j < K; ++j) top.offer(ov[j], oi[j]);
        }
    }
    if (lane == 0) {
        red_m[wave] = m; red_s[wave] = s;
#pragma unroll
        for (int j = 0; j < K; ++j) { red_v[wave * K + j] = top.v[j]; red_i[wave * K + j] = top.i[j]; }
    }
    __syncthreads();
    if (tid == 0) {
        if (want_top)
            for (int w = 1; w < nw; ++w)
                for (int j = 0; j < K; ++j) top.offer(red_v[w * K + j], red_i[w * K + j]);
        const float l = lse_block_finish(m, s, red_m, red_s, nw);
        const int64_t t = a.tok[b];
        const int hp = a.hist_pos ? a.hist_pos[b] : 1;
        const int slot = (int)((((int64_t)hp - 1) % a.ring_len + a.ring_len) % a.ring_len);
        const int64_t o = (int64_t)slot * a.B + b;
        a.lp[o] = (t >= 0 && t < (int64_t)V) ? row[t] - l : NAN;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j < a.top_k) {
                const bool empty = top.i[j] == 0x7fffffff;
                a.top_id[o * K + j] = empty ? -1 : top.i[j];
                a.top_lp[o * K + j] = empty ? -INFINITY : top.v[j] - l;
            }
        }
    }
}

}  // namespace lmi
