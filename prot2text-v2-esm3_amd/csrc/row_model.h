// Where a row's step counter, draw key and emission rule come from: the one thing in which the lock-step entry points
// (p2t_sample_select, p2t_logits_process) and the per-row ones (p2t_sample_select_rows, p2t_logits_process_rows: continuous batching)
// differ.  The kernels of sample_select.hip and logits_process.hip take one of these by value and are otherwise one body.
//   LockStepRows: ONE counter step[0] for the launch; logits row i is engine row i and draws as global row row0 + i; a finished row does
//                 the whole row's work and emits pad at the shared column (greedy_select_kernel's rule, llama_decode.hip).
//   OwnRows:      logits row i is engine row row_map[i] (nullptr: i) with its own counter row_step[r], limit row_limit[r] and key
//                 row_key[r]; a row outside [0, BB) touches nothing; a finished row is left BEFORE its logits row is read -- its counter
//                 no longer moves, so a pad written at it would overwrite its last token -- and only next[r] = pad is written
//                 (greedy_select_rows_kernel's rule).  The exit is block-uniform: every thread reads the same finished[r], which only
//                 this row's own block writes, and only after its last barrier.
#pragma once
#include "common.h"

namespace p2t {

struct LockStepRows {
    const int32_t* step;
    int64_t row0;
    __device__ __forceinline__ int engine_row(int i) const { return i; }
    // -> false: the block leaves now
    __device__ __forceinline__ bool enter(int, const int32_t*, int64_t*, int64_t, int) const { return true; }
    __device__ __forceinline__ int counter(int) const { return step[0]; }
    __device__ __forceinline__ int64_t key(int r) const { return row0 + r; }
    // a finished row emits pad, the token goes to column clamp(step[0]) of out_tokens, a row finishes once it emits an eos id
    __device__ __forceinline__ void emit(int r, int tok_in, int V, const int64_t* __restrict__ eos, int n_eos, int64_t pad,
                                         int32_t* __restrict__ finished, int64_t* __restrict__ next, int64_t* __restrict__ out_tokens,
                                         int64_t ld_tok, int step_now, int Gcap) const {
        int64_t tok = min(max(tok_in, 0), V - 1);
        const int fin = finished[r];
        if (fin) tok = pad;
        next[r] = tok;
        const int st = min(max(step_now, 0), Gcap - 1);
        out_tokens[(int64_t)r * ld_tok + st] = tok;
        if (!fin) {
            for (int e = 0; e < n_eos; ++e)
                if (tok == eos[e]) finished[r] = 1;
        }
    }
};

struct OwnRows {
    const int32_t* row_step;
    const int32_t* row_limit;               // nullptr where nothing is emitted (p2t_logits_process_rows)
    const int32_t* row_map;
    const int64_t* row_key;                 // nullptr where nothing is drawn
    int BB;
    __device__ __forceinline__ int engine_row(int i) const { return row_map ? row_map[i] : i; }
    __device__ __forceinline__ bool enter(int r, const int32_t* finished, int64_t* next, int64_t pad, int tid) const {
        if (r < 0 || r >= BB) return false;
        if (finished && finished[r]) {
            if (next && tid == 0) next[r] = pad;
            return false;
        }
        return true;
    }
    __device__ __forceinline__ int counter(int r) const { return row_step[r]; }
    __device__ __forceinline__ int64_t key(int r) const { return row_key[r]; }
    // the token at the row's own index, then the eos bit (1) and the limit bit (2); the row is live (enter)
    __device__ __forceinline__ void emit(int r, int tok_in, int V, const int64_t* __restrict__ eos, int n_eos, int64_t,
                                         int32_t* __restrict__ finished, int64_t* __restrict__ next, int64_t* __restrict__ out_tokens,
                                         int64_t ld_tok, int step_now, int Gcap) const {
        const int64_t tok = min(max(tok_in, 0), V - 1);
        const int st = min(max(step_now, 0), Gcap - 1);
        next[r] = tok;
        out_tokens[(int64_t)r * ld_tok + st] = tok;
        int fin = 0;
        for (int e = 0; e < n_eos; ++e)
            if (tok == eos[e]) fin |= 1;
        if (st + 1 >= min(max(row_limit[r], 1), Gcap)) fin |= 2;
        if (fin) finished[r] |= fin;
    }
};

}  // namespace p2t
