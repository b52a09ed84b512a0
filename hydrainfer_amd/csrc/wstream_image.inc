// wstream_image.inc — the geometry of a wave's private transpose image, textually included ONCE into each of the four
// weight-streaming kernels (gemm_skinny_kernel, gemm_skinny_fp8w_kernel, moe_gemm_kernel, moe_gemm_fp8w_kernel).
// The image is [16 rows][128 B] = what two load instructions of a wave hold (instruction = 8 rows x 128 B: lane
// (lrow, lpiece) has the 16-byte piece lpiece of row lrow resp. lrow + 8).  The 16-byte slot s of row r is stored at
// slot s ^ ((r >> 1) & 7): row writes (8 lanes x 16 B per row, two rows per 16-lane group) and A-fragment reads
// (lane (r, g) <- row r) are both bank-conflict free.
// Expects in scope: `images` (the LDS address of wave 0's image), `w`, `lrow`, `lpiece`, `r` (lane & 15), `g` (lane >> 4).
// Gives: `tl`, the write offsets `wr_off0` / `wr_off1` of a lane's two pieces, and the A fragment of MFMA step st:
//   a_read16(st), 16-bit weights: 16 bytes, slot 4 st + g of row r;
//   a_read8(st), FP8 weights: 8 bytes, the 8-byte unit 4 st + g of row r = half g & 1 of the slot 2 st + (g >> 1)
// — in both the k of the fragment is 32 st + 8 g .. + 7 of the image's k range, so the x image and its reads are the same.
// (a_read16 forms its whole address where it is used and a_read8 from the three pieces in front of it: that is how the
// kernels were written, and the other way round is other device code.)
char* tl = images + w * 2048;
const int wr_off0 = lrow * 128 + 16 * (lpiece ^ ((lrow >> 1) & 7));
const int wr_off1 = (lrow + 8) * 128 + 16 * (lpiece ^ (((lrow + 8) >> 1) & 7));
[[maybe_unused]] auto a_read16 = [=](int st) {
  return *reinterpret_cast<const u16x8*>(tl + r * 128 + 16 * ((4 * st + g) ^ ((r >> 1) & 7)));
};
[[maybe_unused]] const char* al = tl + r * 128 + 8 * (g & 1);
[[maybe_unused]] const int a_sw = (r >> 1) & 7, a_p = g >> 1;
[[maybe_unused]] auto a_read8 = [=](int st) { return *reinterpret_cast<const u32x2*>(al + 16 * ((2 * st + a_p) ^ a_sw)); };
