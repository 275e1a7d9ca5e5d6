// sample.h — the tail of a SAMPLED decode step: decode_sample_kernel, the sibling of decode_advance_kernel (elementwise.h) that draws
// the token from softmax(logits / T) restricted by top-k and top-p instead of taking the argmax.  Everything else — the token write,
// the history ring, the stop rule, the position / key-count advance, the frozen state of rows with live = 0 — is the same code
// (decode_advance_tail), so the sampled step is the greedy step with a different choice.
//
// Semantics of row b (HF's warper order: temperature, then top-k, then top-p), per-row parameters from device arrays of length B:
//   s_i = logits[b][i] / temperature[b]              (fp32 division; ids in `suppress`, NaN and -inf scores are never drawn)
//   order: s descending, ties by LOWER index first.  Every kept set below is a prefix of this order.
//   top-k (top_k[b] > 0): the first min(k, #allowed) tokens of the order.
//   top-p (top_p[b] < 1): the shortest prefix of the top-k set (of every allowed token when top-k is off) whose mass reaches top_p of
//     the set's mass; at least one token.  Mass of token i = exp(s_i - max s), in fp32, summed in 2^-32 fixed point (uint64), so the
//     sums — and the kept set — do not depend on the order the threads add them in; "reaches" = mass >= ceil(top_p * total mass).
//   draw: exact sampling from the renormalised kept set by Gumbel-max, argmax over kept i of s_i - log(-log u_i) (ties: lower index),
//     u_i = ((x >> 9) + 0.5) * 2^-23 with x the first word of Philox4x32-10 keyed by seed[b] (low word, high word) at the counter
//     (step[b], i, 0, 0).  A row's draw depends only on its seed, its step and its logits row — not on its slot, B, graph or eager.
//   step[b] += live[b] (rows that were live when the step ran).
//
// How (one 1024-thread workgroup per row, as the argmax; the row is 0.5 MB at V = 128 256 and does not fit in LDS, so every pass
// re-reads it from L2 with four 16-byte loads in flight per lane):
//   1. max key (one pass);
//   2. the kept prefix as (tau, cut): tokens whose order-preserving integer key is > tau, plus those == tau with index <= cut.
//      tau comes from a radix select (4 passes of 8-bit digits, 256-bin LDS histograms of counts and fixed-point masses; integer
//      atomics only, so the result is deterministic): by rank for top-k, by cumulative mass for top-p.  `cut` (only when a tie group at
//      tau is split) is a second radix select over the indices of the tied tokens;
//   3. the Gumbel-max pass over the kept tokens (Philox is evaluated for kept tokens only).
// Greedy decoding does not go through here: decode_advance_kernel keeps its own graph and bits.
#pragma once
#include "elementwise.h"

namespace lmi {

struct DecodeSampleArgs {
    DecodeAdvanceArgs adv;        // logits, suppress, tok, pos, k_len, live, budget, eos, hist: as lmi_decode_advance
    const float* temperature;     // [B] > 0
    const int* top_k;             // [B] 0 = off
    const float* top_p;           // [B] >= 1 = off
    const uint64_t* seed;         // [B]
    int* step;                    // [B] Philox counter word 0; += live
};

LMI_DEV uint32_t philox4x32_10_w0(uint64_t seed, uint32_t c0, uint32_t c1) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t x0 = c0, x1 = c1, x2 = 0u, x3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1;
        x1 = (uint32_t)p1; x3 = (uint32_t)p0; x0 = y0; x2 = y2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return x0;
}

// order-preserving key of a scaled score: larger float -> larger key; 0 = never drawn (NaN, -inf)
LMI_DEV uint32_t sample_key(float s) {
    if (!(s > -INFINITY)) return 0u;
    if (s == 0.f) s = 0.f;                                            // -0 and +0 are one value (a tie)
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
LMI_DEV float sample_value(uint32_t key) {
    return __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}
LMI_DEV unsigned long long sample_mass(uint32_t key, float m) {          // exp(s - max) in 2^-32 units, in [0, 2^32]
    return (unsigned long long)(expf(sample_value(key) - m) * 4294967296.0f);
}

// f(v, i) for every i in [0, vocab) of the row: 16 bytes per lane, four loads in flight per thread (decode_advance_kernel's scan)
template <typename F>
LMI_DEV void sample_for_row(const float* row, int vocab, F&& f) {
    const int tid = threadIdx.x;
    const int v4 = ((((size_t)row) & 15) == 0) ? (vocab >> 2) : 0;
    for (int i0 = tid; i0 < v4; i0 += 4 * (int)blockDim.x) {
        f32x4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * (int)blockDim.x;
            q[u] = i < v4 ? *(const f32x4*)(row + 4 * (long)i) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < v4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) f(q[u][e], 4 * i + e);
            }
        }
    }
    for (int i = 4 * v4 + tid; i < vocab; i += blockDim.x) f(row[i], i);
}

struct SampleSel {                // shared state of one radix select
    uint32_t prefix;
    uint32_t rem;                 // rank select: rank still to find inside the chosen bin (after the last level: the ties kept at tau)
    uint32_t last_cnt;            // tokens in the chosen bin of the last level (the tie group at tau)
    uint32_t total_cnt;           // allowed tokens (level 0)
    unsigned long long above_mass, target, total_mass;
};

__global__ void __launch_bounds__(1024) decode_sample_kernel(DecodeSampleArgs a) {
    __shared__ uint32_t h_cnt[256];
    __shared__ unsigned long long h_mass[256];
    __shared__ uint32_t red_k[16];
    __shared__ float best_v[16];
    __shared__ int best_i[16];
    __shared__ SampleSel sel;
    const DecodeAdvanceArgs& d = a.adv;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
    const float* row = d.logits + (long)b * d.ld_logits;
    const float T = a.temperature[b];
    const int top_k = a.top_k[b];
    const float top_p = a.top_p[b];
    auto key_of = [&](float l, int i) -> uint32_t {
        for (int j = 0; j < d.n_suppress; ++j)
            if (d.suppress[j] == i) return 0u;
        return sample_key(l / T);
    };

    // 1. the largest key (the max of s: the mass reference)
    uint32_t mk = 0u;
    sample_for_row(row, d.vocab, [&](float l, int i) { const uint32_t k = key_of(l, i); mk = k > mk ? k : mk; });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)shfl_xor((int)mk, m);
        mk = o > mk ? o : mk;
    }
    if (lane == 0) red_k[wave] = mk;
    __syncthreads();
    for (int w = 0; w < nw; ++w) mk = red_k[w] > mk ? red_k[w] : mk;
    const float smax = sample_value(mk);

    // 2. the kept prefix (tau, cut)
    uint32_t tau = 1u;                                                // every allowed key (> 0) is >= 1: keep all
    int cut = 0x7fffffff;
    // one radix select over `key` (mode 0: rank sel.rem, from the top; mode 1: cumulative mass sel.target, from the top).
    // by_index: select among the tokens with key == tau, by ~index (the rank-th LOWEST index).
    auto radix = [&](int mode, bool by_index, bool want_mass, uint32_t tie_key) {
        for (int lv = 0; lv < 4; ++lv) {
            const int shift = 24 - 8 * lv;
            const uint32_t hi_mask = lv == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int j = tid; j < 256; j += blockDim.x) { h_cnt[j] = 0u; h_mass[j] = 0ull; }
            __syncthreads();
            const uint32_t prefix = sel.prefix;
            sample_for_row(row, d.vocab, [&](float l, int i) {
                uint32_t k = key_of(l, i);
                if (k == 0u) return;
                if (by_index) {
                    if (k != tie_key) return;
                    k = ~(uint32_t)i;
                }
                if ((k & hi_mask) != prefix) return;
                const int dg = (k >> shift) & 255;
                atomicAdd(&h_cnt[dg], 1u);
                if (want_mass) atomicAdd(&h_mass[dg], sample_mass(k, smax));
            });
            __syncthreads();
            if (tid == 0) {
                if (lv == 0) {
                    uint32_t n = 0u;
                    unsigned long long z = 0ull;
                    for (int j = 0; j < 256; ++j) { n += h_cnt[j]; z += h_mass[j]; }
                    sel.total_cnt = n;
                    sel.total_mass = z;
                    if (mode == 0 && sel.rem > n) sel.rem = n;
                    if (mode == 1 && sel.target == 0ull) {            // top-p over everything: the target comes from the total
                        const double t = ceil((double)top_p * (double)z);
                        sel.target = t < 1.0 ? 1ull : (t > (double)z ? z : (unsigned long long)t);
                    }
                }
                int dg = 255;
                for (; dg > 0; --dg) {
                    if (mode == 0 ? (h_cnt[dg] >= sel.rem) : (sel.above_mass + h_mass[dg] >= sel.target)) break;
                    if (mode == 0) sel.rem -= h_cnt[dg];
                    sel.above_mass += h_mass[dg];
                }
                sel.prefix |= (uint32_t)dg << shift;
                sel.last_cnt = h_cnt[dg];
            }
            __syncthreads();
        }
    };
    const bool use_k = top_k > 0, use_p = top_p < 1.f;
    uint32_t n_ties = 0u, eq_cnt = 0u;
    if (mk != 0u && (use_k || use_p)) {
        unsigned long long z_k = 0ull;
        if (use_k) {
            if (tid == 0) { sel.prefix = 0u; sel.rem = (uint32_t)top_k; sel.above_mass = 0ull; sel.target = 0ull; }
            __syncthreads();
            radix(0, false, use_p, 0u);
            tau = sel.prefix; n_ties = sel.rem; eq_cnt = sel.last_cnt;
            z_k = sel.above_mass + (unsigned long long)n_ties * sample_mass(tau, smax);
            __syncthreads();
        }
        if (use_p) {
            if (tid == 0) {
                sel.prefix = 0u; sel.rem = 0u; sel.above_mass = 0ull; sel.target = 0ull;
                if (use_k) {
                    const double t = ceil((double)top_p * (double)z_k);
                    sel.target = t < 1.0 ? 1ull : (t > (double)z_k ? z_k : (unsigned long long)t);
                }
            }
            __syncthreads();
            radix(1, false, true, 0u);
            tau = sel.prefix; eq_cnt = sel.last_cnt;
            const unsigned long long q = sample_mass(tau, smax), need = sel.target - sel.above_mass;      // q > 0: the bin reached the target
            n_ties = (uint32_t)((need + q - 1ull) / q);
            if (n_ties > eq_cnt) n_ties = eq_cnt;
            __syncthreads();
        }
        if (n_ties < eq_cnt) {                                        // a tie group split at tau: keep its n_ties lowest indices
            if (tid == 0) { sel.prefix = 0u; sel.rem = n_ties; sel.above_mass = 0ull; sel.target = 0ull; }
            __syncthreads();
            radix(0, true, false, tau);
            cut = (int)~sel.prefix;
            __syncthreads();
        }
    }

    // 3. Gumbel-max over the kept tokens
    const uint64_t seed = a.seed[b];
    const uint32_t step = (uint32_t)a.step[b];
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    sample_for_row(row, d.vocab, [&](float l, int i) {
        const uint32_t k = key_of(l, i);
        if (k == 0u || k < tau || (k == tau && i > cut)) return;
        const uint32_t x = philox4x32_10_w0(seed, step, (uint32_t)i);
        const float u = ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f);
        const float g = sample_value(k) - logf(-logf(u));
        if (g > bv || (g == bv && i < bi)) { bv = g; bi = i; }
    });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = shfl_xor(bv, m);
        const int oi = shfl_xor(bi, m);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { best_v[wave] = bv; best_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nw; ++w)
            if (best_v[w] > bv || (best_v[w] == bv && best_i[w] < bi)) { bv = best_v[w]; bi = best_i[w]; }
        if (bi == 0x7fffffff) bi = 0;                               // nothing drawable (a row of NaN / -inf only): as decode_advance
        a.step[b] += d.live ? d.live[b] : 1;
        decode_advance_tail(d, b, bi);
    }
}

}  // namespace lmi
