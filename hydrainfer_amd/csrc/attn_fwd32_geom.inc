// attn_fwd32_geom.inc — tile geometry, LDS swizzles and staging map of attn_fwd.hip's two 32x32x16 prefill kernels,
// included at the top of attn_fwd32_kernel and attn_fwd32p_kernel.  Expects T and D in scope.
  constexpr int KS = D / 16;         // QK k-steps
  constexpr int NDB = D / 32;        // 32-dim output blocks
  constexpr int KT = 64;             // keys per tile (two 32-key sub-tiles)
  // LDS images: UNPADDED rows of 2 D bytes with the 16-byte chunks XOR-swizzled per row — the tiles arrive by LDS-DMA
  // (global_load_lds_dwordx4: 64 lanes x 16 bytes land contiguously, so a row cannot be padded; which chunk of its row
  // a lane fetches is free).  Chunk c of row r sits at position c ^ kswz(r) in the K and Q images, c ^ vswz(r) in V:
  //   K / Q, ds_read_b128 of chunk 2 ks + h of rows c = 0 .. 31 (16-lane groups {0-3,12-15,20-27}, ... on 64 banks,
  //     MI355X_MICROARCH.md LDS): the 16 rows of a group need 16 different positions (D = 128: row & 15) resp. 8
  //     different ones per row parity (D = 64, two rows per bank row: (row >> 1) & 7);
  //   V, ds_read_b64_tr_b16 of rows q = 0 .. 3 x 64 bytes (32-lane groups): the four rows go to four different
  //     64-byte quarters of the bank row (D = 128: (row & 3) << 2) resp. two different ones per row parity (D = 64).
  constexpr int RSK = 2 * D, RSV = 2 * D;
  constexpr int LPR = D / 8;
  constexpr int NL = KT * LPR / 256;
  constexpr int KTILE = KT * RSK, VTILE = KT * RSV;
  constexpr int IMG = KTILE + VTILE;       // one tile: K image, V image; two of them
  constexpr int TQ = 128;
  // Staging map of a wave (Q, the K / V tiles, O at the end): instruction j takes rows RPI j .. RPI j + RPI - 1 of the
  // wave's block, D / 8 lanes per row — the whole row contiguous (lane: row RPI j + st_r4, 16-byte chunk st_ch).
  constexpr int RPI = 64 / LPR;         // rows per staging instruction
  constexpr int NQI = 32 / RPI;         // staging instructions per 32-row block of Q / O
  // Tile staging by LDS-DMA: wave w stages the tile's keys 16 w .. 16 w + 15 (a 16-key group never straddles a page:
  // block_size % 16 == 0), instruction j its rows RPI j .. RPI j + RPI - 1 — 1 KiB of the image per instruction, every
  // cache line touched by one instruction.
  static_assert(NL * RPI == 16 && RPI * RSK == 1024, "a wave stages one 16-key group, 1 KiB per instruction");
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][K[KT][RSK] | V[KT][RSV]] | priority flag
  auto kswz = [](int row) { return LPR == 16 ? (row & 15) : ((row >> 1) & 7); };
  auto vswz = [](int row) { return LPR == 16 ? ((row & 3) << 2) : (((row >> 1) & 1) << 2); };
  typedef __attribute__((address_space(4))) const int32_t c_i32;      // read through the scalar cache
  auto tiles_landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, 1>;

  // The O rows leave through LDS (the K / V images are free: every wave has passed the last tile's barrier), so that a
  // store instruction writes whole rows: straight from the accumulator layout — O[query c][dim 32 db + 8 (r >> 2) + 4 hi
  // + (r & 3)] = acc[db][r] / L — each instruction put 16 bytes into each of 32 rows, sixteen such instructions per
  // wave, ~10 us of the 4 x 704 launch by themselves (tools/ablate_attn_prefill32.py, "empty loop" 16.3 us against 6.1
  // without the stores).
  // Unpadded rows with an XOR swizzle of the 8-byte slots (MI355X_MICROARCH.md, LDS): a ds_write_b64 is served in four
  // groups of 16 contiguous lanes on 32 banks — 16 rows at the same column need 16 different slot positions mod 16
  // (slot ^ row does it; a padded stride of 4 banks met pairwise, PMC 6 % of the LDS cycles) — and the ds_read_b128
  // of whole rows in its four non-contiguous groups is conflict-free exactly when the rows are 256 bytes apart.
  // The two halves of that swizzle: each kernel's epilogue writes slot s = 8 db + 2 rq + hi of row r = c at position
  // s ^ r' (r' = r mod D / 8) of the wave's 32-row block ob (as a shared helper that loop changed the ablated
  // instantiations of EXPERIMENTS builds: profiles/attn_fwd32_refactor.md); read back in 16-byte chunks, slots 2 ch,
  // 2 ch + 1 of row r sit in chunk ch ^ (r' >> 1), swapped when r' is odd.
  constexpr int RSO = 2 * D;
  // chunk ch of row rl of the block, in memory order; row = ob + rl * RSO
  auto o_from_lds = [&](const char* row, int rl, int ch) __attribute__((always_inline)) {
    u16x8 v = *reinterpret_cast<const u16x8*>(row + 16 * (ch ^ ((rl & (LPR - 1)) >> 1)));
    if (rl & 1) v = u16x8{v[4], v[5], v[6], v[7], v[0], v[1], v[2], v[3]};
    return v;
  };
