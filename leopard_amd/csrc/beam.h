// beam.h — beam search inside the decode step: the joint choice of K beams over K x V candidates (lmi_beam_step: a row launch and a
// select launch) and the K / V rows of every slot following the beam it descends from (lmi_beam_reorder).  No atomics, no allocation,
// no host synchronisation: all three launches are capturable.
//
// Row launch (beam_rows_kernel): one 512-thread workgroup per live beam row, ONE pass over the RAW fp32 logits row through
// lse_scan_lane / lse_wave_merge / lse_block_finish — the row's lse has the bits of lmi_token_logprobs — while a lane keeps the best 8
// entries it has seen that are neither an eos id nor on the suppress list (TopList: value descending, id ascending, NaN never enters; an
// element is looked up in the two lists only when it would enter the lane's list).  Per row: lse, the first K pairs (id, logit - lse),
// and logit - lse of each eos id (-inf for a suppressed one; an unused or out-of-range eos slot is never a candidate).
//
// Select launch (beam_select_kernel): one wave over the n_rows x (K + MAX_EOS) candidates, total = score[b] + (logit - lse_b) (one fp32
// add).  The order is total descending, then beam ascending, then id ascending — a strict total order; a candidate whose total is NaN
// (a row with a NaN entry, an all -inf row) never enters.  Every lane counts, for its candidates, how many come before it (its rank r)
// and how many of those are not eos (nb).  A non-eos candidate with nb < K becomes next beam nb; a candidate with nb < K (eos or not)
// is entry r of the walk list — the walk ends with the candidate that fills beam K - 1, so its entries are ranks 0 .. n_walk - 1 without
// a gap.  Why this is exact although a row offers only its best K non-eos entries: a non-eos candidate outside its row's best K is
// preceded by K non-eos candidates of that row alone, so the walk has ended before it; every eos candidate is present.
// Beams the candidates cannot fill get tok 0, parent 0, score -inf.
//
// Reorder launch (beam_reorder_kernel): slot b continues from the rows of slot parent[b].  A thread owns one 16-byte chunk of one row
// index of one K or V tensor ACROSS the K slots: it loads the K values into registers, then stores val[parent[b]] into every slot b
// with parent[b] != b — the permutation is in place and free of races by construction (nobody else touches these K chunks).  Rows
// outside [*row0, *rows_held) are never read or written; an identity parent returns after reading it.
//
// lmi_beam_step_rules is lmi_beam_step with HF's logits processors between the log-softmax and the beam scores: its row launch is
// beam_rows_rules_kernel (below, after beam_rows_kernel), its select launch is beam_select_kernel unchanged.
#pragma once
#include "decode_logprob.h"
#include "decode_rules.h"

namespace lmi {

constexpr int kMaxBeams = kMaxTopLogprobs;        // the row kernel's list length
constexpr int kBeamMaxEos = 4;
constexpr int kBeamMaxCand = kMaxBeams * (kMaxBeams + kBeamMaxEos);           // 96
constexpr int kBeamWalkMax = kMaxBeams + kMaxBeams * kBeamMaxEos;             // 40
constexpr int kBeamWalkWords = 5;                 // rank, total (fp32 bits), parent, id, is_eos

struct BeamRowsArgs {
    const float* logits;          // [n_rows, ld] fp32, rows 16-byte aligned
    const int64_t* suppress;      // [n_suppress] nullable
    const int64_t* eos;           // [kBeamMaxEos], entries < 0 unused
    int vocab, ld, n_suppress, K;
    float* row_lse;               // [n_rows]
    int* row_id;                  // [n_rows, 8]   entries j >= K not written; -1 where the row has fewer candidates
    float* row_lp;                // [n_rows, 8]
    float* row_eos_lp;            // [n_rows, kBeamMaxEos]   NaN for an unused slot
};

__global__ void __launch_bounds__(kLogprobThreads) beam_rows_kernel(BeamRowsArgs a) {
    constexpr int NW = kLogprobThreads / 64, K = kMaxTopLogprobs;
    __shared__ float red_m[NW], red_s[NW], red_v[NW * K];
    __shared__ int red_i[NW * K];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
    const float* row = a.logits + (int64_t)b * (int64_t)a.ld;
    const int V = a.vocab;
    int64_t eos[kBeamMaxEos];
#pragma unroll
    for (int j = 0; j < kBeamMaxEos; ++j) eos[j] = a.eos[j];
    auto barred = [&](int i) {                                       // an eos id or a suppressed id: never a continuing candidate
        bool hit = false;
#pragma unroll
        for (int j = 0; j < kBeamMaxEos; ++j) hit = hit || eos[j] == (int64_t)i;
        for (int j = 0; j < a.n_suppress; ++j) hit = hit || a.suppress[j] == (int64_t)i;
        return hit;
    };
    float m = -INFINITY, s = 0.f;
    TopList top;
    top.clear();
    lse_scan_lane(row, V, m, s, [&](float x, int i) {
        if (top_before(x, i, top.v[K - 1], top.i[K - 1]) && !barred(i)) top.insert(x, i);
    });
    lse_wave_merge(m, s);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        float ov[K];
        int oi[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { ov[j] = shfl_xor(top.v[j], k); oi[j] = shfl_xor(top.i[j], k); }
#pragma unroll
        for (int j = 0; j < K; ++j) top.offer(ov[j], oi[j]);
    }
    if (lane == 0) {
        red_m[wave] = m; red_s[wave] = s;
#pragma unroll
        for (int j = 0; j < K; ++j) { red_v[wave * K + j] = top.v[j]; red_i[wave * K + j] = top.i[j]; }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nw; ++w)
            for (int j = 0; j < K; ++j) top.offer(red_v[w * K + j], red_i[w * K + j]);
        const float l = lse_block_finish(m, s, red_m, red_s, nw);
        a.row_lse[b] = l;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j < a.K) {
                const bool empty = top.i[j] == 0x7fffffff;
                a.row_id[b * K + j] = empty ? -1 : top.i[j];
                a.row_lp[b * K + j] = empty ? -INFINITY : top.v[j] - l;
            }
        }
#pragma unroll
        for (int j = 0; j < kBeamMaxEos; ++j) {
            const int64_t e = eos[j];
            float lp = NAN;                                          // unused slot / id outside the vocabulary / a repeat of an earlier slot
            bool use = e >= 0 && e < (int64_t)V;
            for (int q = 0; q < j; ++q) use = use && eos[q] != e;
            if (use) {
                bool sup = false;
                for (int q = 0; q < a.n_suppress; ++q) sup = sup || a.suppress[q] == e;
                lp = sup ? -INFINITY : row[e] - l;
            }
            a.row_eos_lp[b * kBeamMaxEos + j] = lp;
        }
    }
}

// Row launch with the logits processors (beam_rows_rules_kernel, lmi_beam_step_rules).  In beam search transformers applies the processors
// to log_softmax(row), not to the row: s = logit - lse, then the penalty on s, the n-gram ban, the eos ban — so the penalty needs the lse
// FIRST, and the lse is that of the raw row.  Still one pass over the row:
//   1. append   tok[b] joins seq[b] (decode_rules_kernel's rule: the token this step consumes).
//   2. touched  two vocab-bit bitmaps in LDS, built from the ids alone: ``seen`` (ids of the sequence inside [0, vocab); only with a penalty)
//               and ``ban`` (ids that complete a seen n-gram).  No logit is read.
//   3. scan     beam_rows_kernel's pass over the RAW row — the lse has its bits — whose top list also skips the touched ids: among ids no
//               rule touches, s = logit - lse is monotone in the logit, so their best K are found before the lse exists.
//   4. touched  with the lse known, the bitmap words (vocab / 32 of them, not the row) are walked: a touched id that is neither eos nor
//               suppressed offers s' = -inf (banned) or the penalised s (seen) to a second list.
//   5. merge    thread 0: the untouched list as logit - lse and the touched lists through one TopList — (s' descending, id ascending) is a
//               strict total order, so the result is one set whatever the merge order.  The eos values are s' of each eos id: penalised
//               when seen, -inf when banned by an n-gram, suppressed or while min_left[b] > 0; then min_left[b] -= 1.
// A -inf entry is an ordinary candidate that comes last; a row whose lse is NaN or -inf offers nothing (every s is NaN).
struct BeamRulesArgs {
    const int64_t* tok;           // [n_rows] nullable: the token this step consumes
    int* seq;                     // [n_rows, seq_cap]
    int* seq_len;                 // [n_rows]
    const float* penalty;         // [n_rows]
    const int* ngram;             // [n_rows]
    int* min_left;                // [n_rows]
    int seq_cap;
};

__global__ void __launch_bounds__(kLogprobThreads) beam_rows_rules_kernel(BeamRowsArgs a, BeamRulesArgs u) {
    constexpr int NW = kLogprobThreads / 64, K = kMaxTopLogprobs;
    __shared__ uint32_t seen[kRulesMaxVocab / 32], ban[kRulesMaxVocab / 32];
    __shared__ float red_m[NW], red_s[NW], red_v[NW * K];
    __shared__ int red_i[NW * K];
    __shared__ int len_s;
    __shared__ float lse_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6), nt = (int)blockDim.x;
    const float* row = a.logits + (int64_t)b * (int64_t)a.ld;
    int* seq = u.seq + (int64_t)b * (int64_t)u.seq_cap;
    const int V = a.vocab, words = (V + 31) / 32;
    const float p = u.penalty[b];
    const int n = u.ngram[b];
    const int min_left = u.min_left[b];           // read by every thread before the first barrier; written after the last one
    const bool use_p = p != 1.f;
    int64_t eos[kBeamMaxEos];
#pragma unroll
    for (int j = 0; j < kBeamMaxEos; ++j) eos[j] = a.eos[j];
    auto barred = [&](int i) {
        bool hit = false;
#pragma unroll
        for (int j = 0; j < kBeamMaxEos; ++j) hit = hit || eos[j] == (int64_t)i;
        for (int j = 0; j < a.n_suppress; ++j) hit = hit || a.suppress[j] == (int64_t)i;
        return hit;
    };

    // 1. append
    if (tid == 0) {
        int L = u.seq_len[b];
        L = L < 0 ? 0 : (L > u.seq_cap ? u.seq_cap : L);
        if (u.tok && L < u.seq_cap) {
            seq[L] = (int)u.tok[b];
            u.seq_len[b] = ++L;
        }
        len_s = L;
    }
    for (int w = tid; w < words; w += nt) { seen[w] = 0u; ban[w] = 0u; }
    __syncthreads();
    const int L = len_s;

    // 2. the touched ids
    if (use_p) {
        for (int i = tid; i < L; i += nt) {
            const int id = seq[i];
            if (id >= 0 && id < V) atomicOr(&seen[id >> 5], 1u << (id & 31));
        }
    }
    if (n > 0 && L + 1 >= n) {
        const int m = n - 1;                      // the ids to match: seq[L - m .. L)
        const int* tail = seq + (L - m);
        for (int i = tid; i < L - m; i += nt) {
            int k = 0;
            while (k < m && seq[i + k] == tail[k]) ++k;
            if (k < m) continue;
            const int id = seq[i + m];
            if (id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
        }
    }
    __syncthreads();

    // 3. the one pass over the raw row
    float m = -INFINITY, s = 0.f;
    TopList top;
    top.clear();
    lse_scan_lane(row, V, m, s, [&](float x, int i) {
        if (top_before(x, i, top.v[K - 1], top.i[K - 1]) && !(((seen[i >> 5] | ban[i >> 5]) >> (i & 31)) & 1u) && !barred(i)) top.insert(x, i);
    });
    lse_wave_merge(m, s);
    auto wave_top_merge = [&](TopList& t) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
            float ov[K];
            int oi[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { ov[j] = shfl_xor(t.v[j], k); oi[j] = shfl_xor(t.i[j], k); }
#pragma unroll
            for (int j = 0; j < K; ++j) t.offer(ov[j], oi[j]);
        }
    };
    wave_top_merge(top);
    if (lane == 0) {
        red_m[wave] = m; red_s[wave] = s;
#pragma unroll
        for (int j = 0; j < K; ++j) { red_v[wave * K + j] = top.v[j]; red_i[wave * K + j] = top.i[j]; }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nw; ++w)
            for (int j = 0; j < K; ++j) top.offer(red_v[w * K + j], red_i[w * K + j]);
        lse_s = lse_block_finish(m, s, red_m, red_s, nw);
    }
    __syncthreads();                              // the lse is known; red_v / red_i have been read
    const float l = lse_s;

    // 4. the touched ids, from the bitmaps
    auto ruled = [&](int id) {                    // s' of a touched id
        const uint32_t bit = 1u << (id & 31);
        float v = row[id] - l;
        if (seen[id >> 5] & bit) v = v < 0.f ? v * p : v / p;
        if (ban[id >> 5] & bit) v = -INFINITY;
        return v;
    };
    TopList hit;
    hit.clear();
    for (int w = tid; w < words; w += nt) {
        uint32_t bits = seen[w] | ban[w];
        while (bits) {
            const int id = w * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            if (!barred(id)) hit.offer(ruled(id), id);
        }
    }
    wave_top_merge(hit);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) { red_v[wave * K + j] = hit.v[j]; red_i[wave * K + j] = hit.i[j]; }
    }
    __syncthreads();

    // 5. merge and write
    if (tid == 0) {
        TopList fin;
        fin.clear();
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (top.i[j] != 0x7fffffff) fin.offer(top.v[j] - l, top.i[j]);
        for (int w = 0; w < nw; ++w)
            for (int j = 0; j < K; ++j) fin.offer(red_v[w * K + j], red_i[w * K + j]);
        a.row_lse[b] = l;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j < a.K) {
                const bool empty = fin.i[j] == 0x7fffffff;
                a.row_id[b * K + j] = empty ? -1 : fin.i[j];
                a.row_lp[b * K + j] = empty ? -INFINITY : fin.v[j];
            }
        }
#pragma unroll
        for (int j = 0; j < kBeamMaxEos; ++j) {
            const int64_t e = eos[j];
            float lp = NAN;                                          // unused slot / id outside the vocabulary / a repeat of an earlier slot
            bool use = e >= 0 && e < (int64_t)V;
            for (int q = 0; q < j; ++q) use = use && eos[q] != e;
            if (use) {
                bool sup = min_left > 0;
                for (int q = 0; q < a.n_suppress; ++q) sup = sup || a.suppress[q] == e;
                lp = sup ? -INFINITY : ruled((int)e);
            }
            a.row_eos_lp[b * kBeamMaxEos + j] = lp;
        }
        if (min_left > 0) u.min_left[b] = min_left - 1;
    }
}

struct BeamSelectArgs {
    const int* row_id;            // [n_rows, 8]
    const float* row_lp;          // [n_rows, 8]
    const float* row_eos_lp;      // [n_rows, kBeamMaxEos]
    const int64_t* eos;           // [kBeamMaxEos]
    int n_rows, K;
    float* score;                 // [max(n_rows, K)] in: the rows' accumulated log-probabilities; out: the K next beams'
    int64_t* tok;                 // [K] out
    int* parent;                  // [K] out
    int* walk;                    // [1 + kBeamWalkMax * kBeamWalkWords]: n_walk, then (rank, total bits, parent, id, is_eos) per entry
    int* pos;                     // [K] += 1 (nullable)
    int* k_len;                   // [K] += 1 (nullable)
    int* rows_held;               // [1] += 1 (nullable): the rows every slot holds, for lmi_beam_reorder
};

// (t, b, i) comes before (u, c, j): total descending, beam ascending, id ascending
LMI_DEV bool beam_before(float t, int b, int i, float u, int c, int j) { return t > u || (t == u && (b < c || (b == c && i < j))); }

__global__ void __launch_bounds__(64) beam_select_kernel(BeamSelectArgs a) {
    __shared__ float c_tot[kBeamMaxCand];
    __shared__ int c_id[kBeamMaxCand], c_eos[kBeamMaxCand];          // c_id < 0: not a candidate
    const int lane = threadIdx.x, K = a.K, per = K + kBeamMaxEos, n = a.n_rows * per;
    for (int c = lane; c < n; c += 64) {
        const int b = c / per, j = c - b * per;
        float lp;
        int id;
        if (j < K) {
            id = a.row_id[b * kMaxBeams + j];
            lp = a.row_lp[b * kMaxBeams + j];
        } else {
            const int64_t e = a.eos[j - K];
            lp = a.row_eos_lp[b * kBeamMaxEos + (j - K)];
            id = (e >= 0 && e < (int64_t)0x7fffffff) ? (int)e : -1;
        }
        const float t = a.score[b] + lp;
        c_tot[c] = t;
        c_id[c] = (t != t) ? -1 : id;                                // NaN never enters
        c_eos[c] = j >= K;
    }
    __syncthreads();                                                 // every score has been read: the outputs may overwrite them
    int n_walk_mine = 0;
    for (int c = lane; c < n; c += 64) {
        const int id = c_id[c];
        if (id < 0) continue;
        const int b = c / per, is_eos = c_eos[c];
        const float t = c_tot[c];
        int r = 0, nb = 0;
        for (int d = 0; d < n; ++d) {
            const int jd = c_id[d];
            if (jd < 0 || d == c) continue;
            if (beam_before(c_tot[d], d / per, jd, t, b, id)) { ++r; nb += 1 - c_eos[d]; }
        }
        if (nb >= K) continue;                                       // the walk ended before this candidate
        int* w = a.walk + 1 + r * kBeamWalkWords;
        w[0] = r; w[1] = __builtin_bit_cast(int, t); w[2] = b; w[3] = id; w[4] = is_eos;
        n_walk_mine = n_walk_mine > r + 1 ? n_walk_mine : r + 1;
        if (!is_eos) { a.tok[nb] = id; a.parent[nb] = b; a.score[nb] = t; }
    }
    // the walk's length = its last rank + 1; the beams filled = the non-eos candidates in it
    int nw = n_walk_mine;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { const int o = shfl_xor(nw, k); nw = nw > o ? nw : o; }
    int filled = 0;
    for (int c = 0; c < n; ++c) filled += (c_id[c] >= 0 && !c_eos[c]) ? 1 : 0;
    if (filled > K) filled = K;
    if (lane == 0) {
        a.walk[0] = nw;
        if (a.rows_held) a.rows_held[0] += 1;
    }
    if (lane < K) {
        if (lane >= filled) { a.tok[lane] = 0; a.parent[lane] = 0; a.score[lane] = -INFINITY; }
        if (a.pos) a.pos[lane] += 1;
        if (a.k_len) a.k_len[lane] += 1;
    }
}

struct BeamReorderArgs {
    void* const* ptrs;            // [n_tensors] device table of the K / V base pointers
    const int* parent;            // [K]
    const int* row0;              // [1] first row that can differ
    const int* rows_held;         // [1] rows every slot holds
    int K, chunks_per_row;        // 16-byte chunks of one row (rows are contiguous: row stride = row width)
    int slot_rows;                // a slot's capacity in rows: nothing at or past it is touched
    int64_t slot_stride;          // in 16-byte chunks
};

typedef unsigned BeamChunk __attribute__((ext_vector_type(4)));           // 16 bytes, moved as bits

// K is a template parameter: the K chunks and the parent array stay in registers (every index is a compile-time constant)
template <int K>
__global__ void __launch_bounds__(256) beam_reorder_kernel(BeamReorderArgs a) {
    int par[K];
    bool identity = true;
#pragma unroll
    for (int b = 0; b < K; ++b) {
        const int p = a.parent[b];
        par[b] = (p < 0 || p >= K) ? b : p;                          // not a slot: the slot keeps its rows
        identity = identity && par[b] == b;
    }
    if (identity) return;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // chunk index inside [row0, row0 + bound) x chunks_per_row
    const int row0 = a.row0[0];
    const int64_t r = (int64_t)row0 + g / a.chunks_per_row;
    int64_t end = a.rows_held[0];
    if (end > a.slot_rows) end = a.slot_rows;
    if (row0 < 0 || r >= end) return;
    BeamChunk* base = (BeamChunk*)a.ptrs[blockIdx.y] + r * a.chunks_per_row + g % a.chunks_per_row;
    BeamChunk val[K];
#pragma unroll
    for (int s = 0; s < K; ++s) val[s] = base[(int64_t)s * a.slot_stride];
#pragma unroll
    for (int b = 0; b < K; ++b) {
        BeamChunk v = val[0];
#pragma unroll
        for (int s = 1; s < K; ++s)
            if (par[b] == s) v = val[s];
        if (par[b] != b) base[(int64_t)b * a.slot_stride] = v;
    }
}

}  // namespace lmi
