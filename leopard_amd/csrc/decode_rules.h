// decode_rules.h — the logits processors of a decode step (lmi_decode_rules): repetition penalty, no-repeat n-gram ban and
// min_new_tokens, applied IN PLACE to the fp32 logits rows after the head and before the choice kernel (decode_advance_kernel /
// decode_sample_kernel), with the per-sequence state — the ids seen so far, the steps eos stays banned — in device memory, so that the
// launch sits inside the captured step.  HF's processor order: penalty, n-gram ban, minimum length; then the choice kernel's suppress
// list and warpers.
//
// Row b (one 1024-thread workgroup), frozen (nothing read, written or advanced) when live && !live[b]:
//   1. append   tok given and seq_len[b] < seq_cap: seq[b][seq_len[b]] = tok[b], seq_len[b] += 1 — the token this step consumes (the one
//               step t-1 chose) joins the sequence here, so the choice kernels' tail stays as it is.  L = the new length.
//   2. penalty  p = penalty[b] != 1: every id of seq[b][0..L) inside [0, vocab) is rewritten ONCE, l < 0 ? l * p : l / p (one fp32
//               multiply or one IEEE fp32 divide — RepetitionPenaltyLogitsProcessor's torch.where).  "Once" however often the id
//               occurs: a vocab-bit bitmap in LDS, zeroed at entry; threads stride over the sequence and the thread whose atomicOr flips
//               an id's bit from 0 to 1 owns that id's logit.  No pass over the row; the result does not depend on which thread wins.
//   3. n-gram   n = ngram[b] > 0 and L + 1 >= n: for every start i in [0, L - n + 1) whose n - 1 ids equal the last n - 1 ids of the
//               sequence, logits[seq[i + n - 1]] = -inf (NoRepeatNGramLogitsProcessor; n = 1 bans every id seen).  Ids outside
//               [0, vocab) — an image token id — take part in the comparison and are skipped as a write.  After a barrier that follows
//               phase 2, so -inf wins over a penalised value; the writes are idempotent.
//   4. minimum  min_left[b] > 0: logits[eos[j]] = -inf for every used eos id in range, then min_left[b] -= 1.
// NaN and +-inf entries need no special case: -inf * p and -inf / p stay -inf (p > 0), NaN stays NaN.
#pragma once
#include "lmi_device.h"

namespace lmi {

constexpr int kRulesMaxVocab = 262144;            // one bit per id in 32 KB of LDS
constexpr int kRulesThreads = 1024;

struct DecodeRulesArgs {
    float* logits;                // [B, ld] fp32, rewritten in place
    const int64_t* tok;           // [B] nullable: the token this step consumes
    const int* live;              // [B] nullable
    int* seq;                     // [B, seq_cap]
    int* seq_len;                 // [B]
    const float* penalty;         // [B]
    const int* ngram;             // [B]
    int* min_left;                // [B]
    const int64_t* eos;           // [n_eos], entries < 0 unused
    int vocab, ld, seq_cap, n_eos;
};

__global__ void __launch_bounds__(kRulesThreads) decode_rules_kernel(DecodeRulesArgs a) {
    __shared__ uint32_t seen[kRulesMaxVocab / 32];
    __shared__ int len_s;
    const int b = blockIdx.x, tid = threadIdx.x, nt = (int)blockDim.x;
    if (a.live && !a.live[b]) return;
    float* row = a.logits + (int64_t)b * (int64_t)a.ld;
    int* seq = a.seq + (int64_t)b * (int64_t)a.seq_cap;
    const int V = a.vocab;
    const float p = a.penalty[b];
    const int n = a.ngram[b];
    const int min_left = a.min_left[b];           // read by every thread before the first barrier; written after the last one

    // 1. append
    if (tid == 0) {
        int L = a.seq_len[b];
        L = L < 0 ? 0 : (L > a.seq_cap ? a.seq_cap : L);
        if (a.tok && L < a.seq_cap) {
            seq[L] = (int)a.tok[b];
            a.seq_len[b] = ++L;
        }
        len_s = L;
    }
    const bool use_p = p != 1.f;
    if (use_p)
        for (int w = tid; w < (V + 31) / 32; w += nt) seen[w] = 0u;
    __syncthreads();
    const int L = len_s;

    // 2. repetition penalty: the thread that sets an id's bit rewrites its logit
    if (use_p) {
        for (int i = tid; i < L; i += nt) {
            const int id = seq[i];
            if (id < 0 || id >= V) continue;
            const uint32_t bit = 1u << (id & 31);
            if (atomicOr(&seen[id >> 5], bit) & bit) continue;
            const float l = row[id];
            row[id] = l < 0.f ? l * p : l / p;
        }
    }
    __syncthreads();

    // 3. no-repeat n-gram
    if (n > 0 && L + 1 >= n) {
        const int m = n - 1;                      // the ids to match: seq[L - m .. L)
        const int* tail = seq + (L - m);
        for (int i = tid; i < L - m; i += nt) {
            int k = 0;
            while (k < m && seq[i + k] == tail[k]) ++k;
            if (k < m) continue;
            const int id = seq[i + m];
            if (id >= 0 && id < V) row[id] = -INFINITY;
        }
    }

    // 4. min_new_tokens
    if (min_left > 0) {
        for (int j = tid; j < a.n_eos; j += nt) {
            const int64_t e = a.eos[j];
            if (e >= 0 && e < (int64_t)V) row[e] = -INFINITY;
        }
        if (tid == 0) a.min_left[b] = min_left - 1;
    }
}

}  // namespace lmi
