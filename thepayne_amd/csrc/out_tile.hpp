// out_tile.hpp -- what the output layer's plane-operand kernels share (device code only; included by dense_kernels.hpp behind
// DenseParams): the unpacking of the preloaded arguments, a workgroup's 64 x 128 tile, the operand forms with their products, the
// swizzle and a stage's fragments.  Functions and small structs only: the kernels, their schedules, their piece tables and their
// epilogues are in dense_kernels.hpp.  The order of the products is what "the same rows to the bit" between these kernels rests on
// (tests/test_gpu_parity.py, tests/test_out_bits_gpu.py): it is written here and nowhere else.
// Every function here is inlined into kernels whose instruction streams are compared with those of the inline code it replaced
// (NOTES.md): how an argument is passed -- by value, by reference -- is part of that and not a matter of taste.
#pragma once

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// ---- arguments ---------------------------------------------------------------------------------------------------------------------
// (what the prologue's addresses hang off arrives in registers at wave start: the leading scalar parameters, preloaded --
//  -mllvm -amdgpu-kernarg-preload-count; read from the kernarg segment they are 400-700 cycles in front of the first request)
// The kernel's working parameters from the preloaded ones, and the switch to the second output layer (DenseParams::sel: a scalar load
// and a uniform branch; launches without the word skip both), the fp16 forms' row scales with it.
__device__ __forceinline__ void out_args(DenseParams& p, PAYNE_D3_LEAD_PARAMS) {
  p.sel = lead_sel; p.Xp = lead_Xp; p.Wp = lead_Wp; p.plane_x = lead_plane_x; p.plane_w = lead_plane_w;
  p.grid_m = (int)(lead_grid & 0xffffu); p.grid_n = (int)(lead_grid >> 16); p.N = lead_N; p.B = lead_B; p.ldp = lead_ldp; p.K = lead_K;
  if (p.sel != nullptr && (unsigned)*p.sel == lead_sel_seq) {
    p.Wp = p.Wp_alt; p.plane_w = p.plane_w_alt; p.bias = p.bias_alt; p.bias_shift = p.bias_shift_alt; p.N = p.N_alt; p.ldy = p.ldy_alt;
    p.rscale = p.rscale_alt;
  }
}

// ---- a workgroup's tile ------------------------------------------------------------------------------------------------------------
// 64 x 128 outputs, eight waves of 32 x 32 each (2 x 4).  XCD-aware order: blocks b and b+8 share an XCD (round-robin dispatch), so
// give each XCD a contiguous run of tiles (m fastest): its L2 then holds 1/8 of W and all of X.  (n0 >= p.N: the grid was sized for
// the wider of the two output layers -- the kernel returns.)
struct OutTile { int m0, n0; };
__device__ __forceinline__ OutTile out_tile(int grid_m, int ntiles) {        // ntiles = grid_m * grid_n
  int t = blockIdx.x;
  if ((ntiles & 7) == 0) t = (t & 7) * (ntiles >> 3) + (t >> 3);
  return OutTile{(t % grid_m) * 64, (t / grid_m) * 128};
}
// (A wave's 32 x 32 block of it -- lane, wave = readfirstlane(tid >> 6), wm0 = 32 (wave >> 2), wn0 = 32 (wave & 3) -- stays with the
// kernels, behind their early return: how those fold depends on what else a kernel does with the wave's number.)

// ---- operand forms -----------------------------------------------------------------------------------------------------------------
// Three bf16 planes an operand (x = x1 + x2 + x3), six products; two fp16 planes (X = h1 + h2), three: smallest partial products first.
struct Bf16x3 {
  static constexpr int kPlanes = 3;
  typedef bf16x8_t frag_t;
  static __device__ __forceinline__ void products(f32x16& acc, const frag_t (&a)[3], const frag_t (&b)[3]) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
  }
};
struct F16x2 {
  static constexpr int kPlanes = 2;
  typedef f16x8_t frag_t;
  static __device__ __forceinline__ void products(f32x16& acc, const frag_t (&a)[2], const frag_t (&b)[2]) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[0], acc, 0, 0, 0);
  }
};

// ---- a stage's fragments -----------------------------------------------------------------------------------------------------------
// Rows of ROWB bytes (64: a 32-deep stage, 128: 64-deep); 16-byte chunk c of tile row r sits at chunk c ^ out_sw(r): the sixteen lanes
// of every lane group of a fragment read (ds_read_b128) cover sixteen different 16-byte bank groups.
template <int ROWB> __device__ __forceinline__ int out_sw(int row) { return ROWB == 128 ? ((row >> 1) & 7) : ((row >> 2) & 3); }
// The operands of a wave's 32 x 32 block for the ROWB / 32 16-deep matrix steps of a stage.
template <class Form, int ROWB> struct OutFrag { typename Form::frag_t a[ROWB / 32][Form::kPlanes], b[ROWB / 32][Form::kPlanes]; };
// As, Bs: where the stage's A and B blocks start (planes of 64 and B_ROWS rows); Ra, Rb: the lane's rows in them, sa, sb = out_sw of
// them; h = lane >> 5.  (By reference, as the kernels' own lambdas had them: by value the address arithmetic comes out differently.)
template <class Form, int ROWB, int B_ROWS>
__device__ __forceinline__ void out_frags(OutFrag<Form, ROWB>& f, const unsigned char* As, const unsigned char* Bs, const int& Ra, const int& Rb,
                                          const int& sa, const int& sb, const int& h) {
#pragma unroll
  for (int ks = 0; ks < ROWB / 32; ++ks) {
    const int c = 2 * ks + h;
#pragma unroll
    for (int pl = 0; pl < Form::kPlanes; ++pl) {
      f.a[ks][pl] = *reinterpret_cast<const typename Form::frag_t*>(As + pl * (64 * ROWB) + Ra * ROWB + 16 * (c ^ sa));
      f.b[ks][pl] = *reinterpret_cast<const typename Form::frag_t*>(Bs + pl * (B_ROWS * ROWB) + Rb * ROWB + 16 * (c ^ sb));
    }
  }
}
