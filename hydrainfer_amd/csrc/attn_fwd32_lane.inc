// attn_fwd32_lane.inc — the lane's address for the transposed V reads of attn_fwd32_tile.inc, included into
// attn_fwd32_kernel and attn_fwd32p_kernel in front of their tile loops (not part of attn_fwd32_geom.inc: the per-item
// kernel derives its lane maps only after its slot walk).  Expects `lane`, `hi` and attn_fwd32_geom.inc in scope.
  // transposed-read lane address inside a 4-row x 32-dim block: lane 4q + pp of each 16-lane group
  // supplies row q, dims 16 half + 4 pp .. + 3 (half = which 16 of the 32 dims this group takes)
  const int tr_q = (lane & 15) >> 2, tr_pp = lane & 3, tr_half = (lane >> 4) & 1;
  const int tr_off = (4 * hi + tr_q) * RSV + (16 * tr_half + 4 * tr_pp) * 2;      // + 64 * (db ^ tr_x): the swizzled quarter
  const int tr_x = vswz(tr_q) >> 2;
