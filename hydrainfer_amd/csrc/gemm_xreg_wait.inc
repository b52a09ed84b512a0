// gemm_xreg_wait.inc — the waiting half of the NORM = 1 hand-over (protocol: gemm_xreg_produce.inc), textually
// included ONCE into each kernel behind its weight prefetch.  Uses st, cmd, produce of gemm_xreg_produce.inc and the
// kernel's lane, flat_id, p.
// 3. wait for the last row.  Wave 0 polls its XCD's flag line.  RESCUE: a producer workgroup that has
//    not been dispatched yet cannot be waited for if every CU it could get is held by waiters (two
//    processes sharing the GPU, each with such a launch: their workgroups interleave per XCD) — so a
//    workgroup that has waited the rescue bound looks for a row nobody has claimed and computes it itself.
//    Progress therefore needs ONE resident workgroup, not the first M.
for (;;) {
  if (threadIdx.x < 64) {
    const uint32_t* fl = p.sync + 32 * (1 + (__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7));
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    int c = -1;   // -1: flag seen; >= 0: row to rescue; -2: gave up
    while (!__builtin_amdgcn_readfirstlane(__hip_atomic_load(fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
      __builtin_amdgcn_s_sleep(8);
      const uint64_t waited = __builtin_amdgcn_s_memrealtime() - t0;
      if (waited > kRescueTicks && !(p.stagger & 4)) {
        const uint32_t sv = lane < p.M ? __hip_atomic_load(st + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 1u;
        uint64_t free_rows = __ballot(sv == 0u);
        if (free_rows) {
          // rescuers spread over the unclaimed rows (workgroup f takes the (f mod n)-th of them): K missing
          // producers are then rescued side by side, not one after the other through the same lowest row
          for (int skip = flat_id % __builtin_popcountll(free_rows); skip > 0; --skip) free_rows &= free_rows - 1;
          c = __builtin_ctzll(free_rows);
          break;
        }
      }
      // 1 s at 100 MHz: report, never hang the GPU (bit 2 of `stagger`: test hook — no producers, no rescue,
      // 2 ms bound: every norm-fused launch gives up and must be reported by its caller)
      if (waited > ((p.stagger & 4) ? 200000ull : 100000000ull)) {
        if (threadIdx.x == 0) __hip_atomic_fetch_or(p.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = -2;
        break;
      }
    }
    if (threadIdx.x == 0) *cmd = c;
  }
  __syncthreads();
  const int c = *cmd;
  __syncthreads();
  if (c < 0) break;
  produce(c);
}
stamp(2);
asm volatile("" ::: "memory");
