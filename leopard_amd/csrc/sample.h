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
// The steps are device functions (sample_kept_prefix, sample_radix with a key functor, sample_draw) shared with decode_sample_ex_kernel
// below, which adds HF's remaining warpers (min_p, typical_p, epsilon_cutoff, eta_cutoff) between steps 2 and 3.
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

struct SampleLds {                // the LDS of one row's workgroup (both kernels): the two 256-bin histograms and the reduction slots
    uint32_t h_cnt[256];
    unsigned long long h_mass[256];
    uint32_t red_k[16];
    float best_v[16];
    int best_i[16];
    SampleSel sel;
};

struct SampleRow {                // one logits row and what turns an entry into its key
    const float* row;
    int vocab;
    const int64_t* suppress;
    int n_suppress;
    float T;
    LMI_DEV uint32_t key(float l, int i) const {
        for (int j = 0; j < n_suppress; ++j)
            if (suppress[j] == i) return 0u;
        return sample_key(l / T);
    }
};

// the largest of every thread's mk (all threads get it); red_k is free again after the next __syncthreads()
LMI_DEV uint32_t sample_block_max(uint32_t mk, uint32_t* red_k) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)shfl_xor((int)mk, m);
        mk = o > mk ? o : mk;
    }
    if (lane == 0) red_k[wave] = mk;
    __syncthreads();
    for (int w = 0; w < nw; ++w) mk = red_k[w] > mk ? red_k[w] : mk;
    return mk;
}

// One radix select (4 levels of 8-bit digits, from the top) over key(l, i) -> uint32 (0 = not in the set) with mass(l, i, key) per
// token; sel.prefix / rem / above_mass / target are set by the caller.  mode 0: the rank sel.rem; mode 1: the key at which the
// cumulative mass reaches sel.target (target 0: ceil(frac * the set's mass), from level 0).  Integer atomics only.
template <typename KeyF, typename MassF>
LMI_DEV void sample_radix(const SampleRow& R, SampleLds& lds, int mode, bool want_mass, float frac, KeyF&& key, MassF&& mass) {
    const int tid = threadIdx.x;
    SampleSel& sel = lds.sel;
    for (int lv = 0; lv < 4; ++lv) {
        const int shift = 24 - 8 * lv;
        const uint32_t hi_mask = lv == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int j = tid; j < 256; j += blockDim.x) { lds.h_cnt[j] = 0u; lds.h_mass[j] = 0ull; }
        __syncthreads();
        const uint32_t prefix = sel.prefix;
        sample_for_row(R.row, R.vocab, [&](float l, int i) {
            const uint32_t k = key(l, i);
            if (k == 0u) return;
            if ((k & hi_mask) != prefix) return;
            const int dg = (k >> shift) & 255;
            atomicAdd(&lds.h_cnt[dg], 1u);
            if (want_mass) atomicAdd(&lds.h_mass[dg], mass(l, i, k));
        });
        __syncthreads();
        if (tid == 0) {
            if (lv == 0) {
                uint32_t n = 0u;
                unsigned long long z = 0ull;
                for (int j = 0; j < 256; ++j) { n += lds.h_cnt[j]; z += lds.h_mass[j]; }
                sel.total_cnt = n;
                sel.total_mass = z;
                if (mode == 0 && sel.rem > n) sel.rem = n;
                if (mode == 1 && sel.target == 0ull) {                // over everything: the target comes from the total
                    const double t = ceil((double)frac * (double)z);
                    sel.target = t < 1.0 ? 1ull : (t > (double)z ? z : (unsigned long long)t);
                }
            }
            int dg = 255;
            for (; dg > 0; --dg) {
                if (mode == 0 ? (lds.h_cnt[dg] >= sel.rem) : (sel.above_mass + lds.h_mass[dg] >= sel.target)) break;
                if (mode == 0) sel.rem -= lds.h_cnt[dg];
                sel.above_mass += lds.h_mass[dg];
            }
            sel.prefix |= (uint32_t)dg << shift;
            sel.last_cnt = lds.h_cnt[dg];
        }
        __syncthreads();
    }
}

// Steps 1 and 2 of a row: the largest key mk (0: nothing drawable) and the kept prefix after top-k and top-p as (tau, cut)
LMI_DEV void sample_kept_prefix(const SampleRow& R, SampleLds& lds, int top_k, float top_p, uint32_t& mk, uint32_t& tau, int& cut) {
    const int tid = threadIdx.x;
    SampleSel& sel = lds.sel;
    // 1. the largest key (the max of s: the mass reference)
    mk = 0u;
    sample_for_row(R.row, R.vocab, [&](float l, int i) { const uint32_t k = R.key(l, i); mk = k > mk ? k : mk; });
    mk = sample_block_max(mk, lds.red_k);
    const float smax = sample_value(mk);

    // 2. the kept prefix (tau, cut)
    tau = 1u;                                                         // every allowed key (> 0) is >= 1: keep all
    cut = 0x7fffffff;
    // by_index: select among the tokens with key == tie_key, by ~index (the rank-th LOWEST index)
    auto radix = [&](int mode, bool by_index, bool want_mass, uint32_t tie_key) {
        sample_radix(R, lds, mode, want_mass, top_p,
                     [&](float l, int i) -> uint32_t {
                         const uint32_t k = R.key(l, i);
                         if (!by_index || k == 0u) return k;
                         return k != tie_key ? 0u : ~(uint32_t)i;
                     },
                     [&](float, int, uint32_t k) { return sample_mass(k, smax); });
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
}

// Step 3: Gumbel-max over the tokens with keep(key, i) (Philox is evaluated for those only), then the shared tail of the step
template <typename KeepF>
LMI_DEV void sample_draw(const DecodeSampleArgs& a, const SampleRow& R, SampleLds& lds, int b, KeepF&& keep) {
    const DecodeAdvanceArgs& d = a.adv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
    const uint64_t seed = a.seed[b];
    const uint32_t step = (uint32_t)a.step[b];
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    sample_for_row(R.row, R.vocab, [&](float l, int i) {
        const uint32_t k = R.key(l, i);
        if (!keep(k, i)) return;
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
    if (lane == 0) { lds.best_v[wave] = bv; lds.best_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nw; ++w)
            if (lds.best_v[w] > bv || (lds.best_v[w] == bv && lds.best_i[w] < bi)) { bv = lds.best_v[w]; bi = lds.best_i[w]; }
        if (bi == 0x7fffffff) bi = 0;                               // nothing drawable (a row of NaN / -inf only): as decode_advance
        a.step[b] += d.live ? d.live[b] : 1;
        decode_advance_tail(d, b, bi);
    }
}

__global__ void __launch_bounds__(1024) decode_sample_kernel(DecodeSampleArgs a) {
    __shared__ SampleLds lds;
    const DecodeAdvanceArgs& d = a.adv;
    const int b = blockIdx.x;
    const SampleRow R{d.logits + (long)b * d.ld_logits, d.vocab, d.suppress, d.n_suppress, a.temperature[b]};
    uint32_t mk, tau;
    int cut;
    sample_kept_prefix(R, lds, a.top_k[b], a.top_p[b], mk, tau, cut);
    sample_draw(a, R, lds, b, [&](uint32_t k, int i) { return !(k == 0u || k < tau || (k == tau && i > cut)); });
}

// ---- the extended sibling: the rest of HF's warper chain after top-p ----------------------------------------------------------------------
// decode_sample_ex_kernel continues where decode_sample_kernel stops.  S0 = the kept prefix (tau, cut) above; with d_i = s_i - max s and
// w_i = expf(d_i) (fp32), per-row parameters from device arrays of length B (a null array, or a value outside its range, = off; min_p
// above 1 acts as 1), each warper over what the earlier ones left, its softmax renormalised over that set:
//   min_p = m in (0, 1]:          S1 = { i in S0 : w_i >= m }                    (relative to the top token, w = 1, which always stays)
//   typical_p = t in (0, 1):      over S1, Z = sum w, a_i = log Z - d_i (= -log p_i), H = sum p_i a_i, sh_i = |a_i - H| (fp32);
//                                 c = sh of the first token, sh ascending, at which the cumulative mass reaches ceil(t * Z);
//                                 S2 = { i in S1 : sh_i <= c } — whole tie groups at c, a band of scores: the top token can go
//   epsilon_cutoff = e in (0, 1): over S2 with its Z: S3 = { w_i >= e * Z } + the tokens with the largest score of S2
//   eta_cutoff = h in (0, 1):     over S3 with its Z and H: eta = min(h, sqrt(h) * exp(-H)); S4 = { w_i >= eta * Z } + the same top tokens
//   draw: the Gumbel-max of decode_sample_kernel over S4, same Philox counter — with all four off, the same token.
// Z and E = sum w_i * (-d_i) are sums of 2^-32 fixed-point terms (uint64: per-thread, then integer LDS atomics), so they — and the kept
// set — do not depend on the order of the additions; H = log Z + E / Z and the thresholds are computed from them in fp64 by every thread
// alike and rounded to fp32 once.  Passes over the row beyond decode_sample_kernel's: min_p none (a predicate on w), epsilon one (Z),
// eta one (Z, E), typical one (Z, E) plus one four-level select by ~bits(sh) and cumulative mass.  LDS: the same SampleLds (Z and E use
// the two halves of h_mass).
struct DecodeSampleExArgs {
    DecodeSampleArgs s;
    const float* min_p;           // [B] or null
    const float* typical_p;       // [B] or null
    const float* epsilon_cutoff;  // [B] or null
    const float* eta_cutoff;      // [B] or null
};

// Z (sel.total_mass) and E (sel.above_mass) over the tokens with in_set(key, i, w); returns the largest key among them
template <typename SetF>
LMI_DEV uint32_t sample_sums(const SampleRow& R, SampleLds& lds, float smax, SetF&& in_set) {
    const int tid = threadIdx.x;
    for (int j = tid; j < 256; j += blockDim.x) lds.h_mass[j] = 0ull;
    __syncthreads();
    unsigned long long z = 0ull, e = 0ull;
    uint32_t top = 0u;
    sample_for_row(R.row, R.vocab, [&](float l, int i) {
        const uint32_t k = R.key(l, i);
        if (k == 0u) return;
        const float dd = sample_value(k) - smax, w = expf(dd);
        if (!in_set(k, i, w)) return;
        z += (unsigned long long)(w * 4294967296.0f);
        e += (unsigned long long)(w * -dd * 4294967296.0f);
        top = k > top ? k : top;
    });
    atomicAdd(&lds.h_mass[tid & 127], z);
    atomicAdd(&lds.h_mass[128 + (tid & 127)], e);
    top = sample_block_max(top, lds.red_k);                          // (its barrier also orders the atomics before the sums below)
    if (tid == 0) {
        unsigned long long zs = 0ull, es = 0ull;
        for (int j = 0; j < 128; ++j) { zs += lds.h_mass[j]; es += lds.h_mass[128 + j]; }
        lds.sel.total_mass = zs;
        lds.sel.above_mass = es;
    }
    __syncthreads();
    return top;
}

__global__ void __launch_bounds__(1024) decode_sample_ex_kernel(DecodeSampleExArgs x) {
    __shared__ SampleLds lds;
    const DecodeSampleArgs& a = x.s;
    const DecodeAdvanceArgs& d = a.adv;
    const int b = blockIdx.x, tid = threadIdx.x;
    const SampleRow R{d.logits + (long)b * d.ld_logits, d.vocab, d.suppress, d.n_suppress, a.temperature[b]};
    uint32_t mk, tau;
    int cut;
    sample_kept_prefix(R, lds, a.top_k[b], a.top_p[b], mk, tau, cut);
    const float smax = sample_value(mk);

    float m = x.min_p ? x.min_p[b] : 0.f;
    m = m > 0.f ? (m > 1.f ? 1.f : m) : 0.f;
    const float t = x.typical_p ? x.typical_p[b] : 1.f, e = x.epsilon_cutoff ? x.epsilon_cutoff[b] : 0.f, h = x.eta_cutoff ? x.eta_cutoff[b] : 0.f;
    const bool live_row = mk != 0u, use_t = live_row && t > 0.f && t < 1.f, use_e = live_row && e > 0.f && e < 1.f,
               use_h = live_row && h > 0.f && h < 1.f;
    float log_z = 0.f, ent = 0.f, thr_e = 0.f, thr_h = 0.f;            // typical: log Z and H of S1; epsilon / eta: w thresholds (0 = keeps all)
    uint32_t c_key = 0u, top = mk;                                    // typical: ~bits(c) (0 = keeps all); the largest key of S2 (and of S3)
    auto sh_key = [&](uint32_t k) -> uint32_t {
        const float sh = fabsf((log_z - (sample_value(k) - smax)) - ent);
        return ~__builtin_bit_cast(uint32_t, sh);                     // sh ascending = key descending; never 0 (the sign bit of sh is clear)
    };
    auto in1 = [&](uint32_t k, int i, float w) { return !(k < tau || (k == tau && i > cut)) && w >= m; };
    auto in2 = [&](uint32_t k, int i, float w) { return in1(k, i, w) && sh_key(k) >= c_key; };
    auto in3 = [&](uint32_t k, int i, float w) { return in2(k, i, w) && (w >= thr_e || k == top); };
    auto in4 = [&](uint32_t k, int i, float w) { return in3(k, i, w) && (w >= thr_h || k == top); };
    // log Z and H of the set sample_sums just summed (false: the set has no mass in fixed point — its filter is skipped)
    auto stats = [&](double& zf, double& lz, double& hh) {
        const unsigned long long zs = lds.sel.total_mass, es = lds.sel.above_mass;
        zf = (double)zs * (1.0 / 4294967296.0);
        if (zs == 0ull) return false;
        lz = log(zf);
        hh = lz + (double)es / (double)zs;
        return true;
    };
    double zf, lz, hh;
    if (use_t) {
        sample_sums(R, lds, smax, in1);
        if (stats(zf, lz, hh)) {
            log_z = (float)lz; ent = (float)hh;
            __syncthreads();
            if (tid == 0) { lds.sel.prefix = 0u; lds.sel.rem = 0u; lds.sel.above_mass = 0ull; lds.sel.target = 0ull; }
            __syncthreads();
            sample_radix(R, lds, 1, true, t,
                         [&](float l, int i) -> uint32_t {
                             const uint32_t k = R.key(l, i);
                             if (k == 0u) return 0u;
                             return in1(k, i, expf(sample_value(k) - smax)) ? sh_key(k) : 0u;
                         },
                         [&](float l, int, uint32_t) { return sample_mass(sample_key(l / R.T), smax); });
            c_key = lds.sel.prefix;
        }
        __syncthreads();
    }
    if (use_e) {
        top = sample_sums(R, lds, smax, in2);
        if (stats(zf, lz, hh)) thr_e = (float)((double)e * zf);
        __syncthreads();
    }
    if (use_h) {
        top = sample_sums(R, lds, smax, in3);                         // (the top of S3 is the top of S2: in3 reads the old value, or none)
        if (stats(zf, lz, hh)) {
            const double eta = fmin((double)h, sqrt((double)h) * exp(-hh));
            thr_h = (float)(eta * zf);
        }
        __syncthreads();
    }
    sample_draw(a, R, lds, b, [&](uint32_t k, int i) { return k != 0u && in4(k, i, expf(sample_value(k) - smax)); });
}

}  // namespace lmi
