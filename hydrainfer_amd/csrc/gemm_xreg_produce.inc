// gemm_xreg_produce.inc — the producing half of the NORM = 1 hand-over, textually included ONCE into each of the two
// activations-in-registers kernels (gemm_xreg.hip), inside `if (NORM) {`, in front of the kernel's weight prefetch;
// gemm_xreg_wait.inc follows behind the prefetch.  Included text, not a function or a lambda: those forms changed the
// device code of every NORM = 1 kernel (profiles/xreg_handover_refactor.md).
// The including kernel declares in front of it:
//   kNormMaxV, kNormKB   norm_row_256's vectors per virtual thread and slab pieces per round trip
//   mbl                  16-row blocks of the fragment-major x (narrow: the constant MB; wide: ceil(M / 16))
//   n_wg                 workgroups of the launch
//   flat_id, p, smem     the kernel's own
//
// THE PROTOCOL.  x = rms_norm(residual += sum of the slabs) * weight is produced inside the launch that consumes it.
//   Sync area (HX_XREG_SYNC_WORDS words, zeroed by the caller): word 0 rows done, word 1 error, word 32 * (1 + xcc) the
//     flag line of XCD xcc, words kStateWord.. one ownership word per row, words 384.. the time stamps of `stagger` bit 3.
//   Ownership: a row belongs to whoever first exchanges its state word 0 -> 1 (norm_row_256); everybody else stores
//     nothing, so the residual is updated exactly once.  The owner writes x through (sc1), drains its stores, counts
//     the row in, and the one that counts the last row sets all eight flag lines (a single polled line stalls its channel).
//   Progress: workgroup r < M produces row r up front; every workgroup then prefetches weights and wave 0 polls its
//     XCD's flag line.  A workgroup that has waited 30 us (the rescue bound; a normal wait is ~3 us) claims a row nobody
//     has started and produces it itself, so the launch finishes with ONE resident workgroup, not the first M.
//   Bounds: after 1 s (100 MHz clock) a waiter sets the error word and goes on: reported by the caller, never a hang.
//   `stagger` bits (hx_debug_set_option): 1 (xreg_no_producers = 1) nobody produces up front, every row is rescued;
//     2 (xreg_no_producers = 2) no producers and no rescue, the bound is 2 ms: every launch gives up;
//     3 (xreg_timeline) the first and the last workgroup write time stamps of their phases (the kernels' `stamp`).
uint32_t* st = p.sync + kStateWord;
float* red = reinterpret_cast<float*>(smem);
int* cmd = reinterpret_cast<int*>(smem) + 16;
auto produce = [&](int row) {      // whole workgroup; true if this workgroup computed the row
  const bool own = norm_row_256<T, kNormMaxV, MB, kNormKB>(p.nm_partial, p.nm_splits, (int64_t)p.M * p.K,
                                                          reinterpret_cast<u16*>(p.nm_residual),
                                                          reinterpret_cast<const u16*>(p.nm_weight), p.nm_eps, p.K, row,
                                                          const_cast<void*>(p.x), st, red, mbl);
  if (own) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // x is written through: drained = visible
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t old = __hip_atomic_fetch_add(p.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old + 1 == (uint32_t)p.M) {   // last row: one flag line per XCD (a single polled line stalls its channel)
#pragma unroll
        for (int cpy = 0; cpy < 8; ++cpy)
          __hip_atomic_store(p.sync + 32 * (1 + cpy), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  return own;
};
// 1. producers: workgroup r < M computes row r of x FIRST (nothing of its own in flight yet: the row's
//    loads and the store drain are not queued behind weight loads — prefetching first cost the whole gain)
if (flat_id < p.M && !(p.stagger & 6))   // (bit 1 of `stagger`: test hook — nobody produces up front, every row is rescued)
  for (int row = flat_id; row < p.M; row += n_wg) produce(row);   // several rows only when N is tiny
