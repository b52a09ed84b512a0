// logprobs_rounds.inc — the top_k selection rounds of logprobs.hip's kernels: round r writes the row's r-th element in
// hx::arg_better's order and its log-probability.  Included text, not a function (profiles/token_choice_refactor.md).
// In scope: T, src, n, vec, row, top_k, top_ids, top_logprobs, part_v / part_i (two reduction areas), log_sum, and
// round 0's outcome: best and bi (the row's first element, in every thread), cv and ci (this thread's candidate).
float wv = best;
int wi = bi;
for (int r = 0; r < top_k; ++r) {
  if (r > 0) {
    // the previous winner's owner needs its next candidate: its wave finds it together (alone, the owner would walk
    // its 32 elements one after the other while 1023 threads wait: 7 us a round, measured)
    const int nvec8 = (n >> 3) * 8;
    const int owner = vec ? (wi < nvec8 ? (wi >> 3) & (LP_THREADS - 1) : wi - nvec8) : wi & (LP_THREADS - 1);
    if (wi != LP_NONE && (owner >> 6) == (int)(threadIdx.x >> 6)) {
      float nv;
      int ni;
      lp_candidate_of<T>(src, n, vec, owner, wv, wi, nv, ni);
      if ((int)threadIdx.x == owner) { cv = nv; ci = ni; }
    }
    wv = cv;
    wi = ci;
    lp_block_first(wv, wi, part_v[r & 1], part_i[r & 1]);
  }
  if (threadIdx.x == 0) {
    const bool none = wi == LP_NONE;                                    // K > n: the row is used up
    top_ids[row * top_k + r] = none ? -1 : wi;
    top_logprobs[row * top_k + r] = none ? -INFINITY : (wv - best) - log_sum;
  }
}
