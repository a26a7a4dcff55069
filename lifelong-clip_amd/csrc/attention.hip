// Fused multi-head attention core for CLIP towers (d_head = 64), forward and backward.
// Reference semantics: lora.py:950 (q *= d_h^-0.5), 1043 (S = q k^T), 1047-1051 (additive
// -inf causal mask for the text tower, model.py:926-932), 1063 (softmax), 1068 (O = P v); the
// vanilla/adapter towers use torch's nn.MultiheadAttention, same math (model.py:217,230).
//
// Layout: qkv = [rows = batch*L, 3*D] bf16 (q | k | v, head h at columns h*64), as produced by
// the fused QKV GEMM; O = [rows, D] bf16; lse = [batch*H, L] f32 (log2 domain).
//
// MI355X design. Sequences are short (197 image tokens, 77 text tokens): one workgroup owns one
// (sequence, head) pair with the WHOLE key range on chip, one wave per 32 rows (queries or keys),
// keys padded to Lp = 32*NQB (padded keys masked, padded rows zero). At d_head = 64 the
// per-score work is dominated by VALU (scale, max, exp, sum, pack), not MFMA, so the kernels are
// laid out to minimise VALU issue:
//   * LDS images use a row swizzle that is invariant under 16-row steps, so every lane's LDS
//     offsets are computed once; loop steps only add wave-uniform row-block offsets;
//   * masking (padded keys, causal) runs only on the wave-uniform edge blocks, and causal blocks
//     entirely above the diagonal are skipped;
//   * fwd: EXACT softmax in two passes — pass 1 recomputes S^T = K Q^T only for the row max
//     (MFMA is the idle pipe here), pass 2 forms p = exp2(S*c - m*c) with one FMA, packs P^T to
//     bf16 straight from the accumulators into the B operand of O^T = V^T P^T (V^T via
//     ds_read_b64_tr_b16); no online rescaling;
//   * bwd, key-major kernel (dK, dV): each wave keeps its 32 keys' K / V fragments and dK^T, dV^T
//     accumulators in registers and sweeps the queries: S = Q K^T, dP = dO V^T with -D preloaded
//     as the dP accumulator, dS = P * dP, dV^T += dO^T P, dK^T += Q^T dS;
//   * bwd, query-major kernel (dQ): each wave keeps its 32 queries' Q / dO fragments, recomputes
//     S^T, dP^T from K / V in LDS and accumulates dQ^T = K^T dS^T; it walks the heads in reverse
//     order so its reads hit what the key-major kernel left in L2 / the Infinity Cache.
#include "lc_common.h"
#include <type_traits>

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// raw v_exp_f32: arguments are <= 0 here, exp2(-inf) = 0, denormal results flush to 0
LC_DEV float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
// padded key or (text tower) future key; bitwise ops keep it a select, not a branch
LC_DEV bool masked(int key, int q, int L, int causal) {
  return (key >= L) | ((causal != 0) & (key > q));
}

// 128-B-row images: 16-B chunk c of row r lives at chunk c ^ m(r), m(r) = x ^ ((x << 1) & 7) with
// x = (r >> 1) & 7: conflict-free both for row reads (ds_read_b128: lane t reads row t) and for the
// transposed reads (ds_read_b64_tr_b16: 8 rows x 32 B per 32 lanes; the plain x ^ chunk mask put
// rows r and r + 2 on the same banks there, 2-way) — checked exhaustively for every lane group.
// Period 16 rows, so lane offsets stay valid for any 16-row-aligned block.
LC_DEV int swz_mask(int row) {
  const int x = (row >> 1) & 7;
  return x ^ ((x << 1) & 7);
}
LC_DEV int swz(int row, int chunk) { return chunk ^ swz_mask(row); }

LC_DEV bf16x8 lds16(const char* p) { return *reinterpret_cast<const bf16x8*>(p); }
LC_DEV bf16x4 lds_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)(p));
}
LC_DEV bf16x8 cat4(bf16x4 a, bf16x4 b) { return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
LC_DEV bf16x8 as_bf8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
LC_DEV bf16x8 pack8(const f32x4& a, const f32x4& b) {
  return as_bf8(u32x4{pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])});
}

// sum over the 8 lanes of a row (all of them get it)
LC_DEV float sum_row8(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// q / k / v, O and dO rows are read once per (sequence, head): nontemporal (step +0.4 %,
// profiles/r02/epilogue_knockout.txt)
LC_DEV uint4 ld16_or_zero(const bf16_t* p, bool ok) {
  if (!ok) return uint4{0, 0, 0, 0};
  const i32x4 v = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// Raw-buffer descriptor over `rows` rows of `row_bytes` from row row0 of p (wave-uniform): loads
// past the range read zero and stores there are dropped by the range check, so no branch
// surrounds a memory op and hipcc counts vmcnt across them (a load under a branch is followed by
// vmcnt(0): the loads issued before it stop being in flight together).
LC_DEV __amdgpu_buffer_rsrc_t seq_rsrc(const void* p, long row0, long row_bytes, int rows) {
  const uint64_t a = (uint64_t)(static_cast<const char*>(p) + row0 * row_bytes);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const int nb = __builtin_amdgcn_readfirstlane((int)(rows * row_bytes));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
}
LC_DEV uint4 seq_ld16(__amdgpu_buffer_rsrc_t r, int off) {  // nontemporal (read once)
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 2);
  return make_uint4(v[0], v[1], v[2], v[3]);
}
// a buffer offset past every descriptor: the load reads zero (the host's check() keeps every
// offset into a sequence's rows, and every descriptor's size, below it)
constexpr int OOR = 0x7ffffff0;

// Lane offsets (bytes) into a swizzled 128-B-row image, valid for any row block that starts at a
// multiple of 16 rows:
//   row_off(t, g, s): A/B-operand read of row t (+block), k-chunk s*4+g  (16 B)
//   tr_off(t, g, dt): transposed read of rows 4g + (t>>2) (+16 for the upper half), columns
//                     dt*16 + (t&3)*4 .. +3 — the V^T / K^T / Q^T / dO^T fragment layout whose
//                     k order matches a bf16x8 packed from two 16-row accumulator tiles.
LC_DEV int row_off(int t, int g, int s) { return t * 128 + swz(t, s * 4 + g) * 16; }
LC_DEV int tr_off(int t, int g, int dt) {
  const int row = 4 * g + (t >> 2);
  const int col = dt * 16 + (t & 3) * 4;
  return row * 128 + swz(row, col >> 3) * 16 + (col & 7) * 2;
}

// One output row's 64 head columns from the 4 lanes t + 16g that share it (lane g: packed bf16 of
// columns dt*16 + 4g .. +3 in x[dt]) as two 16-B stores per lane instead of four 8-B ones: one
// v_permlane16_swap per dword exchanges lane groups 1 <-> 0 and 3 <-> 2 between the column-tile
// pairs (0, 1) and (2, 3), after which group g holds columns 32p + 16(g & 1) + 8(g >> 1) .. +7
// of pair p (the epilogue store tail is issue-bound: half the store instructions, same bytes).
// All four lanes of the row must be active (row guards are uniform over them).
LC_DEV void store_row64(bf16_t* row, int g, const uint2 (&x)[4]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const auto s0 = __builtin_amdgcn_permlane16_swap(x[2 * p].x, x[2 * p + 1].x, false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(x[2 * p].y, x[2 * p + 1].y, false, false);
    *reinterpret_cast<uint4*>(row + 32 * p + 16 * (g & 1) + 8 * (g >> 1)) =
        uint4{s0[0], s1[0], s0[1], s1[1]};
  }
}

constexpr int V_STRIDE = 160;  // bytes per V row in the forward's plain V image (conflict-free tr)

// ----------------------------------------------------------------------------------- forward
// ONLINE (default): one pass over the keys with a running row max — the O accumulators and row
// sums rescaled by exp2((m_old - m_new) c) per 32-key block — instead of the exact two-pass form
// (a first pass of S = K Q^T for the max alone): a third fewer MFMAs and K reads, image forward
// 103.4 -> 94.8 us standalone (profiles/r03/s2/u_ab_attn_online.txt). LCCLIP_ATTN_FWD_ONLINE=0
// selects the two-pass form (A/Bs).
//
// ROW: one query row per sequence (the image tower's last block: its head reads the CLS row only,
// model.py:782). The same instructions on the same operands as the full launch — every wave
// stages K / V, then only the wave that owns query `row` goes on — so O_row [n_seq, ldo] and
// lse_row [n_seq*H] are bit for bit row `row` of the full launch's O and lse (compact: one output
// row per sequence). K and V are still read whole; the Q reads, 6/7 of the MFMA / exp work and
// the O stores go.
template <int NQB, bool ONLINE = true, bool ROW = false>
__global__ void __launch_bounds__(64 * NQB, 4)
attn_fwd_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                bf16_t* __restrict__ O, long ldo, float* __restrict__ lse, int causal,
                float scale, int row = 0) {
  constexpr int LP = 32 * NQB;
  constexpr int NTH = 64 * NQB;
  __shared__ __attribute__((aligned(16))) char smem[LP * 128 + LP * V_STRIDE];
  char* Ks = smem;
  char* Vs = smem + LP * 128;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, t = lane & 15;
  const int nh = blockIdx.x, n = nh / H, h = nh % H;
  const long base = (long)n * L;
  const float c = scale * LOG2E;

  // staging: every lane issues all its 16-B loads (through the sequence's descriptor: rows >= L
  // read zero) before its first LDS write
  constexpr int IT = LP * 8 / NTH;  // = 4
  const int ch = tid & 7;
  const auto rq = seq_rsrc(qkv, base, ldq * 2, L);
  uint4 kv[IT], vv[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    const int off = r * (int)ldq * 2 + (h * 64 + ch * 8) * 2;
    kv[i] = seq_ld16(rq, off + D * 2);
    vv[i] = seq_ld16(rq, off + D * 4);
  }
  const int qb = 32 * w;
  bf16x8 qf[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = qb + qt * 16 + t;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint4 u = seq_ld16(rq, q * (int)ldq * 2 + (h * 64 + s * 32 + g * 8) * 2);
      qf[qt][s] = *reinterpret_cast<bf16x8*>(&u);
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    *reinterpret_cast<uint4*>(Ks + r * 128 + swz(r, ch) * 16) = kv[i];
    *reinterpret_cast<uint4*>(Vs + r * V_STRIDE + ch * 16) = vv[i];
  }
  __syncthreads();
  if constexpr (ROW) {
    if (w != (row >> 5)) return;  // (no barrier below)
  }

  const char* k0 = Ks + row_off(t, g, 0);
  const char* k1 = Ks + row_off(t, g, 1);
  const char* vt = Vs + (4 * g + (t >> 2)) * V_STRIDE + (t & 3) * 8;
  // key steps holding a key <= the wave's last query (causal) / < L
  const int s_end = causal ? min(NQB, (qb + 31) / 32 + 1) : NQB;

  // S^T tile pair of key step s: lane holds S^T[key = 32s + 16kk + 4g + r][q = qb + 16qt + t]
  auto scores = [&](int s, f32x4 (&S)[2][2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ro = (32 * s + 16 * kk) * 128;
      const bf16x8 ka = lds16(k0 + ro), kb = lds16(k1 + ro);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        S[kk][qt] = mfma16(ka, qf[qt][0], f32x4{0.f, 0.f, 0.f, 0.f});
        S[kk][qt] = mfma16(kb, qf[qt][1], S[kk][qt]);
      }
    }
    if (32 * s + 32 > L || (causal && 32 * s + 31 > qb)) {  // wave-uniform edge block
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            S[kk][qt][r] = masked(32 * s + 16 * kk + 4 * g + r, qb + 16 * qt + t, L, causal)
                               ? -INFINITY : S[kk][qt][r];
    }
  };

  // pass 1: exact row max of the raw scores
  float mx[2] = {-INFINITY, -INFINITY};
#pragma unroll 1
  for (int s = 0; s < (ONLINE ? 0 : s_end); ++s) {
    f32x4 S[2][2];
    scores(s, S);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float m = mx[qt];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        m = fmaxf(fmaxf(m, fmaxf(S[kk][qt][0], S[kk][qt][1])), fmaxf(S[kk][qt][2], S[kk][qt][3]));
      mx[qt] = m;
    }
  }
  float nm[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float m = mx[qt];
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    mx[qt] = m * c;
    nm[qt] = -m * c;
  }

  // pass 2: P = exp2(S*c - m*c), row sums, O^T += V^T P^T
  float sm[2] = {0.f, 0.f};
  f32x4 Oa[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) Oa[dt][0] = Oa[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mr[2] = {-INFINITY, -INFINITY};  // ONLINE: running raw-score max per query
#pragma unroll 1
  for (int s = 0; s < s_end; ++s) {
    f32x4 S[2][2];
    scores(s, S);
    if constexpr (ONLINE) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        float m = fmaxf(fmaxf(fmaxf(S[0][qt][0], S[0][qt][1]), fmaxf(S[0][qt][2], S[0][qt][3])),
                        fmaxf(fmaxf(S[1][qt][0], S[1][qt][1]), fmaxf(S[1][qt][2], S[1][qt][3])));
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float mn = fmaxf(mr[qt], m);  // finite from block 0 on (key 0 is never masked)
        const float corr = ex2((mr[qt] - mn) * c);
        mr[qt] = mn;
        nm[qt] = -mn * c;
        sm[qt] *= corr;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) Oa[dt][qt] *= corr;
      }
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = ex2(__builtin_fmaf(S[kk][qt][r], c, nm[qt]));
          S[kk][qt][r] = p;
          sm[qt] += p;
        }
    const bf16x8 pb0 = pack8(S[0][0], S[1][0]);
    const bf16x8 pb1 = pack8(S[0][1], S[1][1]);
    const char* vs = vt + 32 * s * V_STRIDE;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x8 vf = cat4(lds_tr(vs + dt * 32), lds_tr(vs + 16 * V_STRIDE + dt * 32));
      Oa[dt][0] = mfma16(vf, pb0, Oa[dt][0]);
      Oa[dt][1] = mfma16(vf, pb1, Oa[dt][1]);
    }
  }
  if constexpr (ONLINE) mx[0] = mr[0] * c, mx[1] = mr[1] * c;
  // lane holds O^T[d = dt*16 + 4g + r][q = qb + qt*16 + t]
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float l = sm[qt];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const int q = qb + qt * 16 + t;
    if (ROW ? q == row : q < L) {
      const float inv = 1.0f / l;
      uint2 x[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4 o = Oa[dt][qt];
        x[dt] = uint2{pack2bf(o[0] * inv, o[1] * inv), pack2bf(o[2] * inv, o[3] * inv)};
      }
      store_row64(O + (ROW ? (long)n : base + q) * ldo + h * 64, g, x);
      if (g == 0) lse[ROW ? (long)nh : (long)nh * L + q] = mx[qt] + __log2f(l);
    }
  }
}

// ------------------------------------------------------------------ backward, key-major (dK, dV)
template <int NQB>
__global__ void __launch_bounds__(64 * NQB)
attn_bwd_kv_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                   const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, long ldo,
                   const float* __restrict__ lse, bf16_t* __restrict__ dqkv, long lddq, int causal,
                   float scale) {
  constexpr int LP = 32 * NQB;
  constexpr int NTH = 64 * NQB;
  __shared__ __attribute__((aligned(16))) char smem[2 * LP * 128 + 2 * LP * 4];
  char* Qs = smem;
  char* dOs = smem + LP * 128;
  float* nlse_s = reinterpret_cast<float*>(smem + 2 * LP * 128);  // -lse
  float* nd_s = nlse_s + LP;                                       // -D

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, t = lane & 15;
  const int nh = blockIdx.x, n = nh / H, h = nh % H;
  const long base = (long)n * L;
  const float c = scale * LOG2E;

  // staging: all 16-B loads of Q, dO and O issued before the first LDS write; D = rowsum(dO*O)
  // from the same chunks (8 lanes per row, reduced with xor-shuffles)
  constexpr int IT = LP * 8 / NTH;  // = 4
  const int ch = tid & 7;
  uint4 qv[IT], dv[IT], ov[IT];
  float lv[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    const long off = h * 64 + ch * 8;
    qv[i] = ld16_or_zero(qkv + (base + r) * ldq + off, r < L);
    dv[i] = ld16_or_zero(dO + (base + r) * ldo + off, r < L);
    ov[i] = ld16_or_zero(O + (base + r) * ldo + off, r < L);
    lv[i] = (r < L) ? lse[(long)nh * L + r] : 1e30f;
  }
  // own key block: K / V rows kb + kt2*16 + t, as B-operand fragments
  const int kb = 32 * w;
  bf16x8 kf[2][2], vf[2][2];
#pragma unroll
  for (int kt2 = 0; kt2 < 2; ++kt2) {
    const int key = kb + kt2 * 16 + t;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16_t* src = qkv + (base + key) * ldq + h * 64 + s * 32 + g * 8;
      uint4 ku = ld16_or_zero(src + D, key < L), vu = ld16_or_zero(src + 2 * D, key < L);
      kf[kt2][s] = *reinterpret_cast<bf16x8*>(&ku);
      vf[kt2][s] = *reinterpret_cast<bf16x8*>(&vu);
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    *reinterpret_cast<uint4*>(Qs + r * 128 + swz(r, ch) * 16) = qv[i];
    *reinterpret_cast<uint4*>(dOs + r * 128 + swz(r, ch) * 16) = dv[i];
    const uint32_t aa[4] = {ov[i].x, ov[i].y, ov[i].z, ov[i].w};
    const uint32_t bb[4] = {dv[i].x, dv[i].y, dv[i].z, dv[i].w};
    float dsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      dsum += bf2f(aa[k] & 0xffff) * bf2f(bb[k] & 0xffff) + bf2f(aa[k] >> 16) * bf2f(bb[k] >> 16);
    dsum = sum_row8(dsum);
    if (ch == 0) {
      nd_s[r] = -dsum;
      nlse_s[r] = r < L ? -lv[i] : -1e30f;
    }
  }
  __syncthreads();

  const int ro0 = row_off(t, g, 0), ro1 = row_off(t, g, 1);
  const int tr0 = tr_off(t, g, 0), tr1 = tr_off(t, g, 1), tr2 = tr_off(t, g, 2), tr3 = tr_off(t, g, 3);
  const int tro[4] = {tr0, tr1, tr2, tr3};

  f32x4 dV[4][2], dK[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) dV[dt][k2] = dK[dt][k2] = f32x4{0.f, 0.f, 0.f, 0.f};

  // causal: queries before the block's first key see none of its keys
  const int qc0 = causal ? w : 0;
#pragma unroll 1
  for (int qc = qc0; qc < NQB; ++qc) {
    const bool edge = (kb + 32 > L) || (causal && kb + 31 > qc * 32);
    // B operands (k = 32 queries of this chunk): slot j<4 -> q = 4g+j, j>=4 -> 16+4g+(j-4);
    // one 16-query tile of S / dP is live at a time and packed to bf16 straight away.
    u32x4 pw[2], sw[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int q0 = qc * 32 + qt * 16 + 4 * g;
      const f32x4 nl = *reinterpret_cast<const f32x4*>(nlse_s + q0);
      const f32x4 nd = *reinterpret_cast<const f32x4*>(nd_s + q0);
      const char* qrow = Qs + (qc * 32 + qt * 16) * 128;
      const char* drow = dOs + (qc * 32 + qt * 16) * 128;
      const bf16x8 qa0 = lds16(qrow + ro0), qa1 = lds16(qrow + ro1);
      const bf16x8 da0 = lds16(drow + ro0), da1 = lds16(drow + ro1);
      f32x4 S[2], dP[2];
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        S[k2] = mfma16(qa0, kf[k2][0], f32x4{0.f, 0.f, 0.f, 0.f});
        S[k2] = mfma16(qa1, kf[k2][1], S[k2]);
        dP[k2] = mfma16(da0, vf[k2][0], nd);  // dP - D
        dP[k2] = mfma16(da1, vf[k2][1], dP[k2]);
      }
      // lane holds X[q = q0 + r][key = kb + k2*16 + t]
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = ex2(__builtin_fmaf(S[k2][r], c, nl[r]));
        if (edge) {
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = masked(kb + k2 * 16 + t, q0 + r, L, causal) ? 0.f : p[r];
        }
        const f32x4 ds = p * dP[k2];
        pw[k2][2 * qt] = pack2bf(p[0], p[1]);
        pw[k2][2 * qt + 1] = pack2bf(p[2], p[3]);
        sw[k2][2 * qt] = pack2bf(ds[0], ds[1]);
        sw[k2][2 * qt + 1] = pack2bf(ds[2], ds[3]);
      }
    }
    const bf16x8 pB[2] = {as_bf8(pw[0]), as_bf8(pw[1])};
    const bf16x8 sB[2] = {as_bf8(sw[0]), as_bf8(sw[1])};
    const char* qblk = Qs + qc * 32 * 128;
    const char* dblk = dOs + qc * 32 * 128;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x8 doT = cat4(lds_tr(dblk + tro[dt]), lds_tr(dblk + 16 * 128 + tro[dt]));
      const bf16x8 qT = cat4(lds_tr(qblk + tro[dt]), lds_tr(qblk + 16 * 128 + tro[dt]));
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        dV[dt][k2] = mfma16(doT, pB[k2], dV[dt][k2]);
        dK[dt][k2] = mfma16(qT, sB[k2], dK[dt][k2]);
      }
    }
  }
  // dK, dV of the own key block: lane holds X^T[d = dt*16 + 4g + r][key = kb + k2*16 + t]
#pragma unroll
  for (int k2 = 0; k2 < 2; ++k2) {
    const int key = kb + k2 * 16 + t;
    if (key < L) {
      bf16_t* dst = dqkv + (base + key) * lddq + h * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4 a = dK[dt][k2], b = dV[dt][k2];
        *reinterpret_cast<uint2*>(dst + D + dt * 16 + 4 * g) =
            uint2{pack2bf(a[0] * scale, a[1] * scale), pack2bf(a[2] * scale, a[3] * scale)};
        *reinterpret_cast<uint2*>(dst + 2 * D + dt * 16 + 4 * g) =
            uint2{pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
      }
    }
  }
}

// ------------------------------------------------------------- backward, fused (dK, dV, then dQ)
template <int NQB>
struct BwdLds {
  static constexpr int LP = 32 * NQB;
  static constexpr int DST_STRIDE = LP * 2 + 16;  // bytes per dS^T row (conflict-free tr reads)
  static constexpr int Q_OFF = 0;
  static constexpr int DO_OFF = LP * 128;
  static constexpr int DST_OFF = 2 * LP * 128;
  static constexpr int NLSE_OFF = DST_OFF + LP * DST_STRIDE;
  static constexpr int ND_OFF = NLSE_OFF + LP * 4;
  static constexpr int BYTES = ND_OFF + LP * 4;
};

// Persistent: a workgroup walks (sequence, head) items blockIdx.x, + gridDim.x, ...; the next
// item's Q / dO / O / lse rows and K / V fragments are loaded into registers while the current
// one computes (rows after the current item's LDS image is written, K / V after its phase 1), so
// the item's HBM traffic (~230 KB at L = 197) overlaps the MFMA / exp work of the previous one.
//
// Q8: dQ / dK / dV written as the A operand of the fp8 QKV input-gradient GEMM (MaPLe's fp8
// mode): e4m3 codes (lddq in bytes) + E8M0 scales (q_scale, q_rows), the arithmetic of
// quant_fp8_kernel on the bf16-rounded values, so the codes equal bf16 output + quant_fp8.
//
// ROW: one live query row per sequence (the image tower's compact last block), the result of the
// full kernel on operands blanked off that row — O and dO zero, lse = 1e30 there — from compact
// O / dO [n_seq, ldo] and lse [n_items]; q_rows carries the row index. On such operands every
// query chunk but the live row's adds exact zeros to dK / dV, and every wave's dQ but its owner's
// is zero, so phase 1 runs that chunk alone (its other 31 rows zero in LDS, -lse = -1e30) and
// phase 2 runs on one wave; the others store zero dQ rows. Equal to the full launch up to the
// sign of a zero. LDS holds one chunk of Q / dO / dS^T (BwdLdsRow), so NQB = 8 fits too; there
// the full path is the key-major + query-major pair, whose dQ sums a 32-key block with key
// 16kk + 4g + r in k-slot (g, 4kk + r): phase 2 reads its rows in that order for NQB = 8. That
// pair also sums D = rowsum(dO * O) in two orders (key-major: 8 chunks of 8 columns, pairwise;
// query-major: chunks g and 4 + g in sequence per lane group, then pairwise), so for NQB = 8 the
// dS^T parked for phase 2 comes from a second dP started at the query-major -D.
template <int NQB>
struct BwdLdsRow {
  static constexpr int LP = 32 * NQB;
  static constexpr int DST_STRIDE = 32 * 2 + 16;  // BwdLds<1>'s: one chunk of queries per key row
  static constexpr int Q_OFF = 0;                 // the Q and dO chunks lie inside the K image
  static constexpr int DO_OFF = 32 * 128;
  static constexpr int DST_OFF = LP * 128 > 2 * 32 * 128 ? LP * 128 : 2 * 32 * 128;
  static constexpr int NLSE_OFF = DST_OFF + LP * DST_STRIDE;
  static constexpr int ND_OFF = NLSE_OFF + 32 * 4;
  static constexpr int NDQ_OFF = ND_OFF + 32 * 4;  // NQB = 8: -D in the query-major kernel's order
  static constexpr int BYTES = NDQ_OFF + 32 * 4;
};

template <int NQB, bool PERSIST = (NQB >= 5), bool Q8 = false, bool ROW = false>
__global__ void __launch_bounds__(64 * NQB)
attn_bwd_kernel(int n_items, int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                   const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, long ldo,
                   const float* __restrict__ lse, bf16_t* __restrict__ dqkv, long lddq, int causal,
                   float scale, uint8_t* __restrict__ q_scale = nullptr, long q_rows = 0) {
  static_assert(!(ROW && Q8), "the single-row mode writes 16-bit gradients");
  constexpr int LP = 32 * NQB;
  constexpr int NTH = 64 * NQB;
  using Lay = typename std::conditional<ROW, BwdLdsRow<NQB>, BwdLds<NQB>>::type;
  // ROW: the live row, its chunk, and phase 2's rows of a 32-key block per k-slot half
  const int row = ROW ? (int)q_rows : 0;
  const int rowc = row >> 5;
  constexpr bool KSLOT8 = ROW && NQB == 8;
  constexpr int R_MUL = KSLOT8 ? 4 : 8, R_STEP = KSLOT8 ? 16 : 4;
  __shared__ __attribute__((aligned(16))) char smem[Lay::BYTES];
  char* Qs = smem + Lay::Q_OFF;
  char* dOs = smem + Lay::DO_OFF;
  char* dSTs = smem + Lay::DST_OFF;
  float* nlse_s = reinterpret_cast<float*>(smem + Lay::NLSE_OFF);  // -lse
  float* nd_s = reinterpret_cast<float*>(smem + Lay::ND_OFF);      // -D

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, t = lane & 15;
  const float c = scale * LOG2E;
  int item = blockIdx.x;
  if (item >= n_items) return;

  // staging: 16-B chunks of Q, dO and O rows (8 lanes per row); D = rowsum(dO*O) from the same
  // chunks (xor-shuffles) when they are written to LDS
  // (ROW: the 32 x 8 chunks of the live query chunk, over the first 256 threads' slots)
  constexpr int IT = ROW ? (256 + NTH - 1) / NTH : LP * 8 / NTH;  // full: = 4
  uint4 qv[IT], dv[IT], ov[IT];
  float lv[IT];
  // Every global access of an item goes through a raw-buffer descriptor over that sequence's L
  // rows (wave-uniform): rows >= L fall outside it, so their loads return zero and their stores
  // are dropped by the range check. No branch surrounds a memory op, so hipcc can count vmcnt
  // across them — with a store under a branch it waits vmcnt(0) at the next use of any earlier
  // load, i.e. for every store still in flight (the whole store latency once per item).
  // (ok = false: an empty descriptor — the past-the-end prefetch and the first item's deferred
  // dQ are issued unconditionally and read zeros / store nothing, so their count never depends
  // on a branch either)
  auto rows_rsrc = [&](const void* p, long row0, long row_bytes, bool ok = true) {
    const uint64_t a = (uint64_t)(static_cast<const char*>(p) + (ok ? row0 * row_bytes : 0));
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const int n = __builtin_amdgcn_readfirstlane(ok ? (int)(L * row_bytes) : 0);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
  };
  auto bld16 = [](__amdgpu_buffer_rsrc_t r, int off) {  // nontemporal (read once)
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 2);
    return make_uint4(v[0], v[1], v[2], v[3]);
  };
  // Q rows and lse (prefetched during phase 1), dO and O rows (during phase 2: registers). The
  // per-lane row offsets are recomputed from an opaque copy of tid at every call: hoisted out of
  // the item loop they would stay live through both phases (and spill).
  auto lane_tid = [&]() {
    int v = tid;
    asm volatile("" : "+v"(v));
    return v;
  };
  // ROW: a descriptor over `bytes` bytes at p + off (one compact row, one lse value), and
  // whether slot (thread + i * NTH) of the live chunk's image is a chunk of the live row
  auto span_rsrc = [&](const void* p, long off, int bytes, bool ok) {
    const uint64_t a = (uint64_t)(static_cast<const char*>(p) + (ok ? off : 0));
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const int n = __builtin_amdgcn_readfirstlane(ok ? bytes : 0);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
  };
  auto live_slot = [&](int slot) { return slot < 256 && rowc * 32 + (slot >> 3) == row; };
  auto load_rows = [&](int it_) {
    const int tv = lane_tid();
    const bool ok = it_ < n_items;
    const auto rq = rows_rsrc(qkv, (long)(it_ / H) * L, ldq * 2, ok);
    const int cb = ((it_ % H) * 64 + (tv & 7) * 8) * 2;
    if constexpr (ROW) {
      const auto rl = span_rsrc(lse, (long)it_ * 4, 4, ok);  // this item's one lse value
#pragma unroll
      for (int i = 0; i < IT; ++i) {  // the live row's chunks; every other slot reads zero
        const bool live = live_slot(tv + i * NTH);
        qv[i] = bld16(rq, live ? row * (int)ldq * 2 + cb : OOR);
        lv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rl, live ? 0 : OOR, 0, 0));
      }
    } else {
    const auto rl = rows_rsrc(lse, (long)it_ * L, 4, ok);  // this item's L lse values
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int r = (tv + i * NTH) >> 3;
      qv[i] = bld16(rq, r * (int)ldq * 2 + cb);
      // rows >= L read 0 here; the padded-row value (1e30) is substituted where lv is used
      lv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rl, r * 4, 0, 0));
    }
    }
  };
  auto load_o = [&](int it_) {
    const int tv = lane_tid();
    const bool ok = it_ < n_items;
    const int cb = ((it_ % H) * 64 + (tv & 7) * 8) * 2;
    if constexpr (ROW) {
      const auto rd = span_rsrc(dO, (long)(it_ / H) * ldo * 2, D * 2, ok);  // the compact row
      const auto ro = span_rsrc(O, (long)(it_ / H) * ldo * 2, D * 2, ok);
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const bool live = live_slot(tv + i * NTH);
        dv[i] = bld16(rd, live ? cb : OOR);
        ov[i] = bld16(ro, live ? cb : OOR);
      }
    } else {
    const auto rd = rows_rsrc(dO, (long)(it_ / H) * L, ldo * 2, ok);
    const auto ro = rows_rsrc(O, (long)(it_ / H) * L, ldo * 2, ok);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int r = (tv + i * NTH) >> 3;
      dv[i] = bld16(rd, r * (int)ldo * 2 + cb);
      ov[i] = bld16(ro, r * (int)ldo * 2 + cb);
    }
    }
  };
  // own key block: K / V rows kb + kt2*16 + t, as B-operand fragments
  const int kb = 32 * w;
  bf16x8 kf[2][2], vf[2][2];
  auto load_kv = [&](int it_) {
    const int tv = lane_tid() & 63;
    const auto rq = rows_rsrc(qkv, (long)(it_ / H) * L, ldq * 2, it_ < n_items);
    const int cb = ((it_ % H) * 64 + D + (tv >> 4) * 8) * 2;
#pragma unroll
    for (int kt2 = 0; kt2 < 2; ++kt2) {
      const int key = kb + kt2 * 16 + (tv & 15);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int off = key * (int)ldq * 2 + cb + s * 64;
        uint4 ku = bld16(rq, off), vu = bld16(rq, off + D * 2);
        kf[kt2][s] = *reinterpret_cast<bf16x8*>(&ku);
        vf[kt2][s] = *reinterpret_cast<bf16x8*>(&vu);
      }
    }
  };
  load_rows(item);
  load_o(item);
  load_kv(item);

  // one row's 64 head columns (lane g holds columns dt*16 + 4g + {0..3} in x[dt], the 4 lanes
  // t, t+16, t+32, t+48 share the row) times mul, to dqkv columns col0..col0+63
  // bf16 rows through the sequence's descriptor (row r of the sequence starting at row0; rows
  // >= L dropped by the range check): store_row64's two 16-B pieces per lane
  auto put_row_b = [&](long row0, int r, int col0, f32x4 x0, f32x4 x1, f32x4 x2, f32x4 x3,
                       float mul) {
    const f32x4 x[4] = {x0, x1, x2, x3};
    const auto rs = rows_rsrc(dqkv, row0, lddq * 2, row0 >= 0);
    uint2 xp[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      xp[dt] = uint2{pack2bf(x[dt][0] * mul, x[dt][1] * mul), pack2bf(x[dt][2] * mul, x[dt][3] * mul)};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const auto s0 = __builtin_amdgcn_permlane16_swap(xp[2 * p].x, xp[2 * p + 1].x, false, false);
      const auto s1 = __builtin_amdgcn_permlane16_swap(xp[2 * p].y, xp[2 * p + 1].y, false, false);
      typedef unsigned int v4u __attribute__((ext_vector_type(4)));
      const v4u v = v4u{s0[0], s1[0], s0[1], s1[1]};
#ifdef ATT_KO_STORES  // diagnostic builds only: the stores replaced by a keep-alive (results wrong)
      asm volatile("" ::"v"(v));
      (void)rs;
#else
      __builtin_amdgcn_raw_buffer_store_b128(
          v, rs, r * (int)lddq * 2 + (col0 + 32 * p + 16 * (g & 1) + 8 * (g >> 1)) * 2, 0, 0);
#endif
    }
  };
  auto put_row = [&](long row, int col0, f32x4 x0, f32x4 x1, f32x4 x2, f32x4 x3, float mul) {
    const f32x4 x[4] = {x0, x1, x2, x3};
    if constexpr (!Q8) {
      uint2 xp[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        xp[dt] = uint2{pack2bf(x[dt][0] * mul, x[dt][1] * mul), pack2bf(x[dt][2] * mul, x[dt][3] * mul)};
      store_row64(dqkv + row * lddq + col0, g, xp);
    } else {
      uint8_t* dst = reinterpret_cast<uint8_t*>(dqkv) + row * lddq + col0;
#pragma unroll
      for (int b = 0; b < 2; ++b) {  // 32-column scale blocks: dt = 2b, 2b + 1
        float v[8];
        uint32_t amax = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          v[i] = bf2f(f2bf(x[2 * b + (i >> 2)][i & 3] * mul));
          amax = lc_amax_bits(amax, v[i]);
        }
        amax = max(amax, (uint32_t)__shfl_xor((int)amax, 16));
        amax = max(amax, (uint32_t)__shfl_xor((int)amax, 32));
        const uint32_t byte = e8m0_of_bits(amax);
        const float inv = e8m0_inv(byte);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          *reinterpret_cast<uint32_t*>(dst + (2 * b + j) * 16 + 4 * g) =
              pack4_fp8(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
        if (g == 0) q_scale[fp8_scale_index(row, (col0 >> 5) + b, q_rows)] = (uint8_t)byte;
      }
    }
  };
  // Persistent: item i's dQ rows are stored after item i+1's first barrier, not at the end of
  // item i. CDNA's vmcnt retires loads and stores in issue order, so the wait for the prefetched
  // rows at the top of item i+1 (hipcc emits vmcnt(0) there) would otherwise also wait for the
  // dQ stores issued just before it — their whole latency exposed once per item.
  f32x4 dQp[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dQp[dt][0] = dQp[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  long pbase = -1;
  int ph = 0;
  auto put_dq = [&](long pb, int hh, const f32x4 (&x)[4][2]) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int q = 32 * w + qt * 16 + t;
      if constexpr (!Q8)
        put_row_b(pb, q, hh * 64, x[0][qt], x[1][qt], x[2][qt], x[3][qt], scale);
      else if (pb >= 0 && q < L)
        put_row(pb + q, hh * 64, x[0][qt], x[1][qt], x[2][qt], x[3][qt], scale);
    }
  };
#pragma unroll 1
  for (; item < n_items; item += gridDim.x) {
  const int next = item + gridDim.x;
  const int h = item % H;
  const long base = (long)(item / H) * L;
  const int tvh = lane_tid();  // LDS addresses recomputed per item (hoisted, they spilled)
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tvh + i * NTH) >> 3;  // (ROW: row r of the live chunk, slots past it idle)
    const int ch = tvh & 7;
    if (!ROW || tvh + i * NTH < 256) {
      *reinterpret_cast<uint4*>(Qs + r * 128 + swz(r, ch) * 16) = qv[i];
      *reinterpret_cast<uint4*>(dOs + r * 128 + swz(r, ch) * 16) = dv[i];
    }
    const uint32_t aa[4] = {ov[i].x, ov[i].y, ov[i].z, ov[i].w};
    const uint32_t bb[4] = {dv[i].x, dv[i].y, dv[i].z, dv[i].w};
    float dsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      dsum += bf2f(aa[k] & 0xffff) * bf2f(bb[k] & 0xffff) + bf2f(aa[k] >> 16) * bf2f(bb[k] >> 16);
    dsum += __shfl_xor(dsum, 1);
    dsum += __shfl_xor(dsum, 2);
    dsum += __shfl_xor(dsum, 4);
    if constexpr (KSLOT8) {
      // attn_bwd_q_kernel's D: lane group g adds the column pairs of chunk g, then of chunk
      // 4 + g, in sequence; the groups meet as (g, g ^ 1), then (g, g ^ 2)
      float tk[4], pq = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        tk[k] = bf2f(aa[k] & 0xffff) * bf2f(bb[k] & 0xffff) + bf2f(aa[k] >> 16) * bf2f(bb[k] >> 16);
        pq += tk[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) pq += __shfl_xor(tk[k], 4);  // (meaningful on chunks 0..3)
      pq += __shfl_xor(pq, 1);
      pq += __shfl_xor(pq, 2);
      if (ch == 0 && tvh + i * NTH < 256)
        reinterpret_cast<float*>(smem + Lay::NDQ_OFF)[r] = -pq;
    }
    if constexpr (ROW) {
      if (ch == 0 && tvh + i * NTH < 256) {
        nd_s[r] = -dsum;
        nlse_s[r] = live_slot(tvh + i * NTH) ? -lv[i] : -1e30f;
      }
    } else if (ch == 0) {
      nd_s[r] = -dsum;
      nlse_s[r] = r < L ? -lv[i] : -1e30f;
    }
  }
  __syncthreads();
  if constexpr (PERSIST) {
    put_dq(pbase, ph, dQp);  // the previous item's dQ (see above; none before the first item)
    load_rows(next);         // in flight through phases 1 and 2 (zeros past the last item)
  }

  const int ro0 = row_off(t, g, 0), ro1 = row_off(t, g, 1);
  const int tr0 = tr_off(t, g, 0), tr1 = tr_off(t, g, 1), tr2 = tr_off(t, g, 2), tr3 = tr_off(t, g, 3);
  const int tro[4] = {tr0, tr1, tr2, tr3};

  f32x4 dV[4][2], dK[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) dV[dt][k2] = dK[dt][k2] = f32x4{0.f, 0.f, 0.f, 0.f};

  // causal: queries before the block's first key see none of its keys
  const int qc0 = causal ? w : 0;
  // (ROW: the live row's chunk alone — the other chunks' products are exact zeros)
  const int qc_lo = ROW ? max(qc0, rowc) : qc0, qc_hi = ROW ? rowc + 1 : NQB;
#pragma unroll 1
  for (int qc = qc_lo; qc < qc_hi; ++qc) {
    const bool edge = (kb + 32 > L) || (causal && kb + 31 > qc * 32);
    const int lq = ROW ? 0 : qc * 32;  // the chunk's first row in the LDS images
    // B operands (k = 32 queries of this chunk): slot j<4 -> q = 4g+j, j>=4 -> 16+4g+(j-4);
    // one 16-query tile of S / dP is live at a time and packed to bf16 straight away.
    u32x4 pw[2], sw[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int q0 = qc * 32 + qt * 16 + 4 * g;
      const int lq0 = lq + qt * 16 + 4 * g;
      const f32x4 nl = *reinterpret_cast<const f32x4*>(nlse_s + lq0);
      const f32x4 nd = *reinterpret_cast<const f32x4*>(nd_s + lq0);
      const char* qrow = Qs + (lq + qt * 16) * 128;
      const char* drow = dOs + (lq + qt * 16) * 128;
      const bf16x8 qa0 = lds16(qrow + ro0), qa1 = lds16(qrow + ro1);
      const bf16x8 da0 = lds16(drow + ro0), da1 = lds16(drow + ro1);
      f32x4 S[2], dP[2];
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        S[k2] = mfma16(qa0, kf[k2][0], f32x4{0.f, 0.f, 0.f, 0.f});
        S[k2] = mfma16(qa1, kf[k2][1], S[k2]);
        dP[k2] = mfma16(da0, vf[k2][0], nd);  // dP - D
        dP[k2] = mfma16(da1, vf[k2][1], dP[k2]);
      }
      f32x4 dPq[2];  // (ROW, NQB = 8: dP from the query-major -D, for the parked dS^T)
      if constexpr (KSLOT8) {
        const f32x4 ndq = *reinterpret_cast<const f32x4*>(
            reinterpret_cast<const float*>(smem + Lay::NDQ_OFF) + lq0);
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          dPq[k2] = mfma16(da0, vf[k2][0], ndq);
          dPq[k2] = mfma16(da1, vf[k2][1], dPq[k2]);
        }
      }
      // lane holds X[q = q0 + r][key = kb + k2*16 + t]
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = ex2(__builtin_fmaf(S[k2][r], c, nl[r]));
        if (edge) {
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = masked(kb + k2 * 16 + t, q0 + r, L, causal) ? 0.f : p[r];
        }
        const f32x4 ds = p * dP[k2];
        pw[k2][2 * qt] = pack2bf(p[0], p[1]);
        pw[k2][2 * qt + 1] = pack2bf(p[2], p[3]);
        sw[k2][2 * qt] = pack2bf(ds[0], ds[1]);
        sw[k2][2 * qt + 1] = pack2bf(ds[2], ds[3]);
        // park dS^T[key][q0..q0+3] for the dQ phase
        uint2 park = uint2{sw[k2][2 * qt], sw[k2][2 * qt + 1]};
        if constexpr (KSLOT8) {
          const f32x4 dsq = p * dPq[k2];
          park = uint2{pack2bf(dsq[0], dsq[1]), pack2bf(dsq[2], dsq[3])};
        }
        *reinterpret_cast<uint2*>(dSTs + (kb + k2 * 16 + t) * Lay::DST_STRIDE + lq0 * 2) = park;
      }
    }
    const bf16x8 pB[2] = {as_bf8(pw[0]), as_bf8(pw[1])};
    const bf16x8 sB[2] = {as_bf8(sw[0]), as_bf8(sw[1])};
    const char* qblk = Qs + lq * 128;
    const char* dblk = dOs + lq * 128;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x8 doT = cat4(lds_tr(dblk + tro[dt]), lds_tr(dblk + 16 * 128 + tro[dt]));
      const bf16x8 qT = cat4(lds_tr(qblk + tro[dt]), lds_tr(qblk + 16 * 128 + tro[dt]));
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        dV[dt][k2] = mfma16(doT, pB[k2], dV[dt][k2]);
        dK[dt][k2] = mfma16(qT, sB[k2], dK[dt][k2]);
      }
    }
  }
  // dK, dV of the own key block: lane holds X^T[d = dt*16 + 4g + r][key = kb + k2*16 + t]
#pragma unroll
  for (int k2 = 0; k2 < 2; ++k2) {
    const int key = kb + k2 * 16 + t;
    if constexpr (!Q8) {
      put_row_b(base, key, D + h * 64, dK[0][k2], dK[1][k2], dK[2][k2], dK[3][k2], scale);
      put_row_b(base, key, 2 * D + h * 64, dV[0][k2], dV[1][k2], dV[2][k2], dV[3][k2], 1.0f);
    } else if (key < L) {  // every lane of the row (same t) takes this branch together
      put_row(base + key, D + h * 64, dK[0][k2], dK[1][k2], dK[2][k2], dK[3][k2], scale);
      put_row(base + key, 2 * D + h * 64, dV[0][k2], dV[1][k2], dV[2][k2], dV[3][k2], 1.0f);
    }
  }
  __syncthreads();  // every wave is done with Qs -> reuse it for K
  char* Ks = Qs;
#pragma unroll
  for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int key = kb + kt2 * 16 + t;
      *reinterpret_cast<bf16x8*>(Ks + key * 128 + swz(key, s * 4 + g) * 16) = kf[kt2][s];
    }
  if constexpr (PERSIST) {  // kf / vf, phase-1 accumulators dead until the next item
    load_o(next);
    load_kv(next);
  }
  __syncthreads();

  // phase 2: dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q] for queries qb..qb+31 (k order:
  // key = 32s + 8g + j, from rows 8g+(t>>2) and 8g+4+(t>>2) of both images)
  // (ROW: the live chunk's wave alone; its dS^T columns start at 0. R_MUL / R_STEP: see ROW)
  const int qb = 32 * w;
  const int s_end = (ROW && w != rowc) ? 0 : (causal ? min(NQB, w + 1) : NQB);
  int klo[4], khi[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const int col = dt * 16 + (t & 3) * 4;
    const int r0 = R_MUL * g + (t >> 2);
    klo[dt] = r0 * 128 + swz(r0, col >> 3) * 16 + (col & 7) * 2;
    khi[dt] = (r0 + R_STEP) * 128 + swz(r0 + R_STEP, col >> 3) * 16 + (col & 7) * 2;
  }
  const char* dst0 = dSTs + (R_MUL * g + (t >> 2)) * Lay::DST_STRIDE + ((ROW ? 0 : qb) + (t & 3) * 4) * 2;
  f32x4 dQ[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dQ[dt][0] = dQ[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int s = 0; s < s_end; ++s) {
    const char* ds = dst0 + 32 * s * Lay::DST_STRIDE;
    const bf16x8 bq0 = cat4(lds_tr(ds), lds_tr(ds + R_STEP * Lay::DST_STRIDE));
    const bf16x8 bq1 = cat4(lds_tr(ds + 32), lds_tr(ds + R_STEP * Lay::DST_STRIDE + 32));
    const char* kblk = Ks + 32 * s * 128;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x8 ka = cat4(lds_tr(kblk + klo[dt]), lds_tr(kblk + khi[dt]));
      dQ[dt][0] = mfma16(ka, bq0, dQ[dt][0]);
      dQ[dt][1] = mfma16(ka, bq1, dQ[dt][1]);
    }
  }
  if constexpr (!PERSIST) {  // one item per workgroup (short sequences: many workgroups)
    put_dq(base, h, dQ);
    break;
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dQp[dt][0] = dQ[dt][0], dQp[dt][1] = dQ[dt][1];
  pbase = base;
  ph = h;
  __syncthreads();  // phase 2 done with Ks / dS^T before the next item's LDS image
  }
  if (PERSIST && pbase >= 0) put_dq(pbase, ph, dQp);
}

// ------------------------------------------------------------------ backward, query-major (dQ)
template <int NQB>
__global__ void __launch_bounds__(64 * NQB, 4)
attn_bwd_q_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                  const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, long ldo,
                  const float* __restrict__ lse, bf16_t* __restrict__ dqkv, long lddq, int causal,
                  float scale) {
  constexpr int LP = 32 * NQB;
  constexpr int NTH = 64 * NQB;
  __shared__ __attribute__((aligned(16))) char smem[2 * LP * 128];
  char* Ks = smem;
  char* Vs = smem + LP * 128;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, t = lane & 15;
  // reverse order: the key-major kernel touched the last heads most recently (L2 / Infinity Cache)
  const int nh = gridDim.x - 1 - blockIdx.x, n = nh / H, h = nh % H;
  const long base = (long)n * L;
  const float c = scale * LOG2E;

  constexpr int IT = LP * 8 / NTH;  // = 4
  const int ch = tid & 7;
  uint4 kv[IT], vv[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    const bf16_t* src = qkv + (base + r) * ldq + h * 64 + ch * 8;
    kv[i] = ld16_or_zero(src + D, r < L);
    vv[i] = ld16_or_zero(src + 2 * D, r < L);
  }
  const int qb = 32 * w;
  bf16x8 qf[2][2], df[2][2];
  float nl[2], nd[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = qb + qt * 16 + t;
    float dsum = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const long off = h * 64 + s * 32 + g * 8;
      uint4 u = ld16_or_zero(qkv + (base + q) * ldq + off, q < L);
      uint4 d = ld16_or_zero(dO + (base + q) * ldo + off, q < L);
      uint4 o = ld16_or_zero(O + (base + q) * ldo + off, q < L);
      qf[qt][s] = *reinterpret_cast<bf16x8*>(&u);
      df[qt][s] = *reinterpret_cast<bf16x8*>(&d);
      const uint32_t oo[4] = {o.x, o.y, o.z, o.w}, dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        dsum += bf2f(oo[k] & 0xffff) * bf2f(dd[k] & 0xffff) + bf2f(oo[k] >> 16) * bf2f(dd[k] >> 16);
    }
    dsum += __shfl_xor(dsum, 16);
    dsum += __shfl_xor(dsum, 32);
    nd[qt] = -dsum;
    nl[qt] = q < L ? -lse[(long)nh * L + q] : -1e30f;
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    *reinterpret_cast<uint4*>(Ks + r * 128 + swz(r, ch) * 16) = kv[i];
    *reinterpret_cast<uint4*>(Vs + r * 128 + swz(r, ch) * 16) = vv[i];
  }
  __syncthreads();

  const int ro0 = row_off(t, g, 0), ro1 = row_off(t, g, 1);
  const int tro[4] = {tr_off(t, g, 0), tr_off(t, g, 1), tr_off(t, g, 2), tr_off(t, g, 3)};
  const int s_end = causal ? min(NQB, (qb + 31) / 32 + 1) : NQB;

  f32x4 dQ[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dQ[dt][0] = dQ[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int s = 0; s < s_end; ++s) {
    const bool edge = (32 * s + 32 > L) || (causal && 32 * s + 31 > qb);
    // one 16-key tile of S^T / dP^T live at a time, packed to bf16 straight away
    u32x4 sw[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ro = (32 * s + 16 * kk) * 128;
      const bf16x8 ka0 = lds16(Ks + ro + ro0), ka1 = lds16(Ks + ro + ro1);
      const bf16x8 va0 = lds16(Vs + ro + ro0), va1 = lds16(Vs + ro + ro1);
      f32x4 S[2], dP[2];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        S[qt] = mfma16(ka0, qf[qt][0], f32x4{0.f, 0.f, 0.f, 0.f});
        S[qt] = mfma16(ka1, qf[qt][1], S[qt]);
        dP[qt] = mfma16(va0, df[qt][0], f32x4{nd[qt], nd[qt], nd[qt], nd[qt]});
        dP[qt] = mfma16(va1, df[qt][1], dP[qt]);
      }
      // lane holds X^T[key = 32s + 16kk + 4g + r][q = qb + qt*16 + t]
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = ex2(__builtin_fmaf(S[qt][r], c, nl[qt]));
        if (edge) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            p[r] = masked(32 * s + 16 * kk + 4 * g + r, qb + qt * 16 + t, L, causal) ? 0.f : p[r];
        }
        const f32x4 ds = p * dP[qt];
        sw[qt][2 * kk] = pack2bf(ds[0], ds[1]);
        sw[qt][2 * kk + 1] = pack2bf(ds[2], ds[3]);
      }
    }
    const bf16x8 sb0 = as_bf8(sw[0]);
    const bf16x8 sb1 = as_bf8(sw[1]);
    const char* kblk = Ks + 32 * s * 128;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x8 kT = cat4(lds_tr(kblk + tro[dt]), lds_tr(kblk + 16 * 128 + tro[dt]));
      dQ[dt][0] = mfma16(kT, sb0, dQ[dt][0]);
      dQ[dt][1] = mfma16(kT, sb1, dQ[dt][1]);
    }
  }
  // lane holds dQ^T[d = dt*16 + 4g + r][q = qb + qt*16 + t]
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = qb + qt * 16 + t;
    if (q < L) {
      bf16_t* dst = dqkv + (base + q) * lddq + h * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4 a = dQ[dt][qt];
        *reinterpret_cast<uint2*>(dst + dt * 16 + 4 * g) =
            uint2{pack2bf(a[0] * scale, a[1] * scale), pack2bf(a[2] * scale, a[3] * scale)};
      }
    }
  }
}

// ------------------------------------------------ backward, two-phase (dQ, then dK / dV), 2 per CU
// One workgroup per (sequence, head), NQB waves; wave w owns the 16-row blocks w and w + NQB
// (its queries in phase 1, its keys in phase 2). LDS holds one pair of row images at a time
// (K | V, then Q | dO) plus the -lse / -D rows: 59 KB at L <= 224, so two workgroups share a CU
// and one's loads and stores run under the other's MFMA / exp chain. The fused kernel parks
// the whole dS^T (163 KB: one workgroup per CU, 1.75 waves per SIMD, its memory instructions
// exposed: profiles/r03/j_attn_bwd_knockouts.txt). The price is S and dP formed twice.
//   phase 1 (query-major, attn_bwd_q_kernel's math): S^T = K Q^T, dP^T = V dO^T - D from the
//     K / V images and the wave's Q / dO fragments; dQ^T += K^T dS^T.
//   hand-over: each wave reads its key blocks' K / V fragments from the images, then writes its
//     query blocks' Q / dO fragments as the Q / dO images (every row is one wave's block).
//   phase 2 (key-major, attn_bwd_kv_kernel's math on 16-key blocks): S = Q K^T,
//     dP = dO V^T - D; dV^T += dO^T P, dK^T += Q^T dS.
template <int NQB, bool CAUSAL>
__global__ void __launch_bounds__(64 * NQB) __attribute__((amdgpu_waves_per_eu(4)))
attn_bwd2_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                 const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, long ldo,
                 const float* __restrict__ lse, bf16_t* __restrict__ dqkv, long lddq, float scale,
                 int ko) {
  constexpr int causal = CAUSAL;
  // non-causal: both query / key chunk loops fully unrolled (LDS offsets in the instructions,
  // the edge chunk known at compile time); causal: runtime bounds, rolled
  constexpr int UNR = CAUSAL ? 1 : NQB;
  // ko: timing knockouts of DIAG builds (LC_ATT2_KO; results wrong), 0 otherwise: 1 no phase-1
  // loop, 2 no phase-2 loop, 4 stores replaced by keep-alives, 8 every item loads item 0's rows
  constexpr int LP = 32 * NQB;
  constexpr int NTH = 64 * NQB;
  __shared__ __attribute__((aligned(16))) char smem[2 * LP * 128 + 2 * LP * 4];
  char* I0 = smem;             // K rows, then Q rows
  char* I1 = smem + LP * 128;  // V rows, then dO rows
  float* nlse_s = reinterpret_cast<float*>(smem + 2 * LP * 128);  // -lse
  float* nd_s = nlse_s + LP;                                       // -D

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar block bounds
  const int g = lane >> 4, t = lane & 15;
  const int nh = blockIdx.x, n = nh / H, h = nh % H;
  const long base = (long)n * L;
  const float c = scale * LOG2E;

  // every global load first, through raw-buffer descriptors over this sequence's L rows (rows
  // >= L read zeros from the range check: no branch around a load, so no vmcnt(0) between them):
  // K / V rows for the images, then the wave's two query blocks' Q / dO fragments (B operands
  // of S^T / dP^T: lane holds row q = qb + t, columns s*32 + 8g ..), O rows and lse
  const long lb = (ko & 8) ? 0 : base;
  const int hl = (ko & 8) ? 0 : h;
  const auto rq = seq_rsrc(qkv, lb, ldq * 2, L);
  const auto rd = seq_rsrc(dO, lb, ldo * 2, L);
  const auto rO = seq_rsrc(O, lb, ldo * 2, L);
  const auto rl = seq_rsrc(lse, (ko & 8) ? 0 : (long)nh * L, 4, L);
  constexpr int IT = LP * 8 / NTH;  // = 4
  const int ch = tid & 7;
  uint4 kv[IT], vv[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    const int off = r * (int)ldq * 2 + (hl * 64 + ch * 8) * 2;
    kv[i] = seq_ld16(rq, off + D * 2);
    vv[i] = seq_ld16(rq, off + D * 4);
  }
  bf16x8 qf[2][2], df[2][2];
  uint4 of[2][2];
  float lv[2];
#pragma unroll
  for (int bk = 0; bk < 2; ++bk) {
    const int q = 16 * (w + NQB * bk) + t;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int cb = (hl * 64 + s * 32 + g * 8) * 2;
      uint4 u = seq_ld16(rq, q * (int)ldq * 2 + cb);
      uint4 d = seq_ld16(rd, q * (int)ldo * 2 + cb);
      of[bk][s] = seq_ld16(rO, q * (int)ldo * 2 + cb);
      qf[bk][s] = *reinterpret_cast<bf16x8*>(&u);
      df[bk][s] = *reinterpret_cast<bf16x8*>(&d);
    }
    lv[bk] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rl, q * 4, 0, 0));
    asm volatile("" : "+v"(lv[bk]));  // issued here, not sunk into the q < L select below
  }
  float nl[2], nd[2];
#pragma unroll
  for (int bk = 0; bk < 2; ++bk) {
    const int q = 16 * (w + NQB * bk) + t;
    float dsum = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 d8 = df[bk][s];
      const u32x4 dd = __builtin_bit_cast(u32x4, d8);
      const uint32_t oo[4] = {of[bk][s].x, of[bk][s].y, of[bk][s].z, of[bk][s].w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        dsum += bf2f(oo[k] & 0xffff) * bf2f(dd[k] & 0xffff) + bf2f(oo[k] >> 16) * bf2f(dd[k] >> 16);
    }
    dsum += __shfl_xor(dsum, 16);
    dsum += __shfl_xor(dsum, 32);
    nd[bk] = -dsum;
    nl[bk] = q < L ? -lv[bk] : -1e30f;
    if (g == 0) {  // phase 2 reads every query's -lse / -D from LDS
      nd_s[q] = nd[bk];
      nlse_s[q] = nl[bk];
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * NTH) >> 3;
    *reinterpret_cast<uint4*>(I0 + r * 128 + swz(r, ch) * 16) = kv[i];
    *reinterpret_cast<uint4*>(I1 + r * 128 + swz(r, ch) * 16) = vv[i];
  }
  __syncthreads();

  const int ro0 = row_off(t, g, 0), ro1 = row_off(t, g, 1);
  const int tro[4] = {tr_off(t, g, 0), tr_off(t, g, 1), tr_off(t, g, 2), tr_off(t, g, 3)};

  // ---- phase 1: dQ of the wave's query blocks
#pragma unroll
  for (int bk = 0; bk < 2; ++bk) {
    const int qb = 16 * (w + NQB * bk);
    if (qb >= L) continue;  // wave-uniform
    const int s_end = (ko & 1) ? 0 : causal ? (qb + 15) / 32 + 1 : NQB;
    f32x4 dQ[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dQ[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll UNR
    for (int s = 0; s < NQB; ++s) {
      if (s >= s_end) break;
      const bool edge = (32 * s + 32 > L) || (causal && 32 * s + 31 > qb);
      // one 16-key tile of S^T / dP^T live at a time, packed to bf16 straight away; k slots of
      // the dS^T operand: j < 4 -> key 32s + 4g + j, j >= 4 -> 32s + 16 + 4g + (j - 4)
      u32x4 sw;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ro = (32 * s + 16 * kk) * 128;
        const bf16x8 ka0 = lds16(I0 + ro + ro0), ka1 = lds16(I0 + ro + ro1);
        const bf16x8 va0 = lds16(I1 + ro + ro0), va1 = lds16(I1 + ro + ro1);
        f32x4 S = mfma16(ka0, qf[bk][0], f32x4{0.f, 0.f, 0.f, 0.f});
        S = mfma16(ka1, qf[bk][1], S);
        f32x4 dP = mfma16(va0, df[bk][0], f32x4{nd[bk], nd[bk], nd[bk], nd[bk]});
        dP = mfma16(va1, df[bk][1], dP);
        // lane holds X^T[key = 32s + 16kk + 4g + r][q = qb + t]
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = ex2(__builtin_fmaf(S[r], c, nl[bk]));
        if (edge) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            p[r] = masked(32 * s + 16 * kk + 4 * g + r, qb + t, L, causal) ? 0.f : p[r];
        }
        const f32x4 ds = p * dP;
        sw[2 * kk] = pack2bf(ds[0], ds[1]);
        sw[2 * kk + 1] = pack2bf(ds[2], ds[3]);
      }
      const bf16x8 sb = as_bf8(sw);
      const char* kblk = I0 + 32 * s * 128;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 kT = cat4(lds_tr(kblk + tro[dt]), lds_tr(kblk + 16 * 128 + tro[dt]));
        dQ[dt] = mfma16(kT, sb, dQ[dt]);
      }
    }
    // lane holds dQ^T[d = dt*16 + 4g + r][q = qb + t]
    const int q = qb + t;
    if (q < L) {  // the 4 lanes of the row agree
      uint2 x[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        x[dt] = uint2{pack2bf(dQ[dt][0] * scale, dQ[dt][1] * scale),
                      pack2bf(dQ[dt][2] * scale, dQ[dt][3] * scale)};
      if (ko & 4)
        asm volatile("" ::"v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]));
      else
        store_row64(dqkv + (base + q) * lddq + h * 64, g, x);
    }
  }

  // ---- hand-over: K / V fragments of the wave's key blocks (B operands of S = Q K^T,
  // dP = dO V^T: lane holds row key = kb + t, columns s*32 + 8g ..), then the Q / dO images
  bf16x8 kf[2][2], vf[2][2];
#pragma unroll
  for (int bk = 0; bk < 2; ++bk) {
    const int kb = 16 * (w + NQB * bk);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      kf[bk][s] = lds16(I0 + kb * 128 + (s ? ro1 : ro0));
      vf[bk][s] = lds16(I1 + kb * 128 + (s ? ro1 : ro0));
    }
  }
  __syncthreads();  // every wave holds its K / V fragments
#pragma unroll
  for (int bk = 0; bk < 2; ++bk) {
    const int qb = 16 * (w + NQB * bk);  // rows >= L: zeros (loaded so)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      *reinterpret_cast<bf16x8*>(I0 + qb * 128 + (s ? ro1 : ro0)) = qf[bk][s];
      *reinterpret_cast<bf16x8*>(I1 + qb * 128 + (s ? ro1 : ro0)) = df[bk][s];
    }
  }
  __syncthreads();

  // ---- phase 2: dK, dV of the wave's key blocks
#pragma unroll
  for (int bk = 0; bk < 2; ++bk) {
    const int kb = 16 * (w + NQB * bk);
    if (kb >= L) continue;  // wave-uniform
    f32x4 dV[4], dK[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dV[dt] = dK[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int qc0 = (ko & 2) ? NQB : causal ? kb / 32 : 0;  // (causal: earlier queries see none of it)
#pragma unroll UNR
    for (int qc = 0; qc < NQB; ++qc) {
      if (qc < qc0) continue;
      const bool edge = (kb + 16 > L) || (causal && kb + 15 > qc * 32);
      // k slots of the P / dS operands: j < 4 -> q = 32qc + 4g + j, j >= 4 -> 32qc + 16 + 4g + j-4
      u32x4 pw, sw;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int q0 = qc * 32 + qt * 16 + 4 * g;
        const f32x4 nlv = *reinterpret_cast<const f32x4*>(nlse_s + q0);
        const f32x4 ndv = *reinterpret_cast<const f32x4*>(nd_s + q0);
        const int ro = (qc * 32 + qt * 16) * 128;
        const bf16x8 qa0 = lds16(I0 + ro + ro0), qa1 = lds16(I0 + ro + ro1);
        const bf16x8 da0 = lds16(I1 + ro + ro0), da1 = lds16(I1 + ro + ro1);
        f32x4 S = mfma16(qa0, kf[bk][0], f32x4{0.f, 0.f, 0.f, 0.f});
        S = mfma16(qa1, kf[bk][1], S);
        f32x4 dP = mfma16(da0, vf[bk][0], ndv);
        dP = mfma16(da1, vf[bk][1], dP);
        // lane holds X[q = q0 + r][key = kb + t]
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = ex2(__builtin_fmaf(S[r], c, nlv[r]));
        if (edge) {
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = masked(kb + t, q0 + r, L, causal) ? 0.f : p[r];
        }
        const f32x4 ds = p * dP;
        pw[2 * qt] = pack2bf(p[0], p[1]);
        pw[2 * qt + 1] = pack2bf(p[2], p[3]);
        sw[2 * qt] = pack2bf(ds[0], ds[1]);
        sw[2 * qt + 1] = pack2bf(ds[2], ds[3]);
      }
      const bf16x8 pB = as_bf8(pw), sB = as_bf8(sw);
      const char* qblk = I0 + qc * 32 * 128;
      const char* dblk = I1 + qc * 32 * 128;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 doT = cat4(lds_tr(dblk + tro[dt]), lds_tr(dblk + 16 * 128 + tro[dt]));
        const bf16x8 qT = cat4(lds_tr(qblk + tro[dt]), lds_tr(qblk + 16 * 128 + tro[dt]));
        dV[dt] = mfma16(doT, pB, dV[dt]);
        dK[dt] = mfma16(qT, sB, dK[dt]);
      }
    }
    // lane holds X^T[d = dt*16 + 4g + r][key = kb + t]
    const int key = kb + t;
    if (key < L) {
      uint2 xk[4], xv[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        xk[dt] = uint2{pack2bf(dK[dt][0] * scale, dK[dt][1] * scale),
                       pack2bf(dK[dt][2] * scale, dK[dt][3] * scale)};
        xv[dt] = uint2{pack2bf(dV[dt][0], dV[dt][1]), pack2bf(dV[dt][2], dV[dt][3])};
      }
      bf16_t* dst = dqkv + (base + key) * lddq + h * 64;
      if (ko & 4) {
        asm volatile("" ::"v"(xk[0]), "v"(xk[1]), "v"(xk[2]), "v"(xk[3]));
        asm volatile("" ::"v"(xv[0]), "v"(xv[1]), "v"(xv[2]), "v"(xv[3]));
      } else {
        store_row64(dst + D, g, xk);
        store_row64(dst + 2 * D, g, xv);
      }
    }
  }
}

// -------------------------------------------------- one query row per sequence: the backward
// The image tower's head reads the CLS row of the last block only (model.py:782), so that block's
// attention has one live query per (sequence, head) (forward: attn_fwd_kernel<.., ROW>). Its
// backward is L dot products of 64 and rank-1 updates: memory-bound (K and V of every key are
// read, all of dq | dk | dv written), plain f32 VALU, no MFMA.
// One workgroup of 4 waves per (sequence, head); 8 lanes share a key row (lane ch holds its 16-B
// chunk ch), 32 rows per pass, ROW_IT passes cover L <= 256. Every K / V load of a lane is issued
// before its first use; rows >= L read zero through the sequence's descriptor and their stores
// are dropped by its range check.
constexpr int ROW_NTH = 256;
constexpr int ROW_IT = 8;

LC_DEV void unpack8(uint4 u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = bf2f(w[k] & 0xffff);
    f[2 * k + 1] = bf2f(w[k] >> 16);
  }
}
LC_DEV float dot8(const float (&a)[8], const float (&b)[8]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s = __builtin_fmaf(a[j], b[j], s);
  return s;
}
// sum over the 8 rows of a wave's pass
LC_DEV float sum_rows8(float v) {
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
typedef unsigned int row_v4u __attribute__((ext_vector_type(4)));

// dO is zero off `row`: dv_j = p_j dO, dk_j = scale dS_j q, dq_row = scale sum_j dS_j k_j with
// dS_j = p_j (dO . v_j - dO . O); every other dq row, and dk / dv of the keys the row does not
// see, are written as zeros (all L rows of the sequence's dq | dk | dv are written).
__global__ void __launch_bounds__(ROW_NTH)
attn_row_bwd_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq, int row,
                    const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, long ldo,
                    const float* __restrict__ lse, bf16_t* __restrict__ dqkv, long lddq, int causal,
                    float scale) {
  __shared__ float red_q[4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ch = tid & 7, r0 = tid >> 3;
  const int nh = blockIdx.x, n = nh / H, h = nh % H;
  const float c = scale * LOG2E;
  const auto rq = seq_rsrc(qkv, (long)n * L, ldq * 2, L);
  const auto rs = seq_rsrc(dqkv, (long)n * L, lddq * 2, L);
  const int cb = (h * 64 + ch * 8) * 2;
  uint4 kv[ROW_IT], vv[ROW_IT];
#pragma unroll
  for (int i = 0; i < ROW_IT; ++i) {
    const int off = (r0 + 32 * i) * (int)ldq * 2 + cb;
    kv[i] = seq_ld16(rq, off + D * 2);
    vv[i] = seq_ld16(rq, off + D * 4);
  }
  float qf[8], df[8], of[8];
  unpack8(seq_ld16(rq, row * (int)ldq * 2 + cb), qf);
  unpack8(*reinterpret_cast<const uint4*>(dO + (long)n * ldo + h * 64 + ch * 8), df);
  unpack8(*reinterpret_cast<const uint4*>(O + (long)n * ldo + h * 64 + ch * 8), of);
  const float delta = sum_row8(dot8(df, of));
  const float nl = -lse[nh];
  const int last = causal ? row : L - 1;
  const int oob = L * (int)lddq * 2;  // an offset the descriptor's range check drops

  float dqa[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dqa[j] = 0.f;
#pragma unroll
  for (int i = 0; i < ROW_IT; ++i) {
    const int r = r0 + 32 * i;
    float kf[8], vf[8];
    unpack8(kv[i], kf);
    unpack8(vv[i], vf);
    const float sc = sum_row8(dot8(qf, kf));
    const float dp = sum_row8(dot8(df, vf));
    const bool seen = r <= last;
    const float p = seen ? ex2(__builtin_fmaf(sc, c, nl)) : 0.f;
    // attn_bwd_kernel's rounding points: P and dS enter their products in the storage type
    const float ds = seen ? bf2f(f2bf(p * (dp - delta))) : 0.f;
    const float pr = bf2f(f2bf(p));
    const float dss = ds * scale;
    row_v4u wk, wv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dqa[2 * k] = __builtin_fmaf(ds, kf[2 * k], dqa[2 * k]);
      dqa[2 * k + 1] = __builtin_fmaf(ds, kf[2 * k + 1], dqa[2 * k + 1]);
      wk[k] = seen ? pack2bf(dss * qf[2 * k], dss * qf[2 * k + 1]) : 0u;
      wv[k] = seen ? pack2bf(pr * df[2 * k], pr * df[2 * k + 1]) : 0u;
    }
    const int off = r * (int)lddq * 2 + cb;
    __builtin_amdgcn_raw_buffer_store_b128(wk, rs, off + D * 2, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(wv, rs, off + D * 4, 0, 0);
    // dq: zero off the row (the row itself is stored after the reduction, by the same lanes)
    __builtin_amdgcn_raw_buffer_store_b128(row_v4u{0u, 0u, 0u, 0u}, rs, r != row ? off : oob, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) dqa[j] = sum_rows8(dqa[j]);
  if (lane < 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red_q[w][ch * 8 + j] = dqa[j];
  }
  __syncthreads();
  if (r0 == (row & 31)) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      x[j] = ((red_q[0][ch * 8 + j] + red_q[1][ch * 8 + j]) +
              (red_q[2][ch * 8 + j] + red_q[3][ch * 8 + j])) * scale;
    *reinterpret_cast<uint4*>(dqkv + ((long)n * L + row) * lddq + h * 64 + ch * 8) =
        uint4{pack2bf(x[0], x[1]), pack2bf(x[2], x[3]), pack2bf(x[4], x[5]), pack2bf(x[6], x[7])};
  }
}

// ------------------------------------------------------------- long family, 257 <= L <= 512 keys
// NCH = ceil(L / 32) = 9..16 chunks, LP = 32 * NCH padded rows. One workgroup of 8 waves per
// (sequence, head) with the whole key (backward, key-major: query) range in LDS; wave w walks the
// 32-row chunks w and w + 8 one after the other. Each chunk's body is that of the one-wave-per-
// chunk kernels above — attn_fwd_kernel's online pass, attn_bwd_kv_kernel's query sweep,
// attn_bwd_q_kernel's key sweep, the same rounding points — so a wave's register demand is that
// of their 8-chunk instances. LDS: forward K + V images LP * 288 B (82 944 .. 147 456), key-major
// Q + dO + -lse + -D LP * 264 B (<= 135 168), query-major K + V LP * 256 B (<= 131 072): one
// workgroup per CU, which is what bounds residency (no minimum-occupancy argument).
// Staging is ceil(LP * 8 / 512) passes of 512 16-B pieces, rows guarded against LP (an odd NCH
// leaves the last pass half full); the swizzle's 16-row period keeps the lane offsets valid.
constexpr int LONG_NTH = 512, LONG_WAVES = 8;

template <int NCH>
__global__ void __launch_bounds__(LONG_NTH)
attn_long_fwd_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                     bf16_t* __restrict__ O, long ldo, float* __restrict__ lse, int causal,
                     float scale) {
  constexpr int LP = 32 * NCH;
  __shared__ __attribute__((aligned(16))) char smem[LP * 128 + LP * V_STRIDE];
  char* Ks = smem;
  char* Vs = smem + LP * 128;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, t = lane & 15;
  const int nh = blockIdx.x, n = nh / H, h = nh % H;
  const long base = (long)n * L;
  const float c = scale * LOG2E;

  // staging through the sequence's descriptor: rows >= L read zero, rows >= LP are not written
  constexpr int IT = (LP * 8 + LONG_NTH - 1) / LONG_NTH;
  const int ch = tid & 7;
  const auto rq = seq_rsrc(qkv, base, ldq * 2, L);
  uint4 kv[IT], vv[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * LONG_NTH) >> 3;
    const int off = r * (int)ldq * 2 + (h * 64 + ch * 8) * 2;  // (r <= 511: check())
    kv[i] = seq_ld16(rq, off + D * 2);
    vv[i] = seq_ld16(rq, off + D * 4);
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * LONG_NTH) >> 3;
    if (r < LP) {
      *reinterpret_cast<uint4*>(Ks + r * 128 + swz(r, ch) * 16) = kv[i];
      *reinterpret_cast<uint4*>(Vs + r * V_STRIDE + ch * 16) = vv[i];
    }
  }
  __syncthreads();

  const char* k0 = Ks + row_off(t, g, 0);
  const char* k1 = Ks + row_off(t, g, 1);
  const char* vt = Vs + (4 * g + (t >> 2)) * V_STRIDE + (t & 3) * 8;

#pragma unroll 1
  for (int qc = w; qc < NCH; qc += LONG_WAVES) {  // (no barrier below)
    const int qb = 32 * qc;
    bf16x8 qf[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int q = qb + qt * 16 + t;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint4 u = seq_ld16(rq, q * (int)ldq * 2 + (h * 64 + s * 32 + g * 8) * 2);
        qf[qt][s] = *reinterpret_cast<bf16x8*>(&u);
      }
    }
    // key steps holding a key <= the chunk's last query (causal) / < L
    const int s_end = causal ? min(NCH, qc + 1) : NCH;

    float sm[2] = {0.f, 0.f}, nm[2] = {0.f, 0.f};
    f32x4 Oa[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) Oa[dt][0] = Oa[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mr[2] = {-INFINITY, -INFINITY};  // running raw-score max per query
#pragma unroll 1
    for (int s = 0; s < s_end; ++s) {
      // S^T tile pair: lane holds S^T[key = 32s + 16kk + 4g + r][q = qb + 16qt + t]
      f32x4 S[2][2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ro = (32 * s + 16 * kk) * 128;
        const bf16x8 ka = lds16(k0 + ro), kb = lds16(k1 + ro);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          S[kk][qt] = mfma16(ka, qf[qt][0], f32x4{0.f, 0.f, 0.f, 0.f});
          S[kk][qt] = mfma16(kb, qf[qt][1], S[kk][qt]);
        }
      }
      if (32 * s + 32 > L || (causal && 32 * s + 31 > qb)) {  // wave-uniform edge block
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              S[kk][qt][r] = masked(32 * s + 16 * kk + 4 * g + r, qb + 16 * qt + t, L, causal)
                                 ? -INFINITY : S[kk][qt][r];
      }
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        float m = fmaxf(fmaxf(fmaxf(S[0][qt][0], S[0][qt][1]), fmaxf(S[0][qt][2], S[0][qt][3])),
                        fmaxf(fmaxf(S[1][qt][0], S[1][qt][1]), fmaxf(S[1][qt][2], S[1][qt][3])));
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float mn = fmaxf(mr[qt], m);  // finite from block 0 on (key 0 is never masked)
        const float corr = ex2((mr[qt] - mn) * c);
        mr[qt] = mn;
        nm[qt] = -mn * c;
        sm[qt] *= corr;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) Oa[dt][qt] *= corr;
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = ex2(__builtin_fmaf(S[kk][qt][r], c, nm[qt]));
            S[kk][qt][r] = p;
            sm[qt] += p;
          }
      const bf16x8 pb0 = pack8(S[0][0], S[1][0]);
      const bf16x8 pb1 = pack8(S[0][1], S[1][1]);
      const char* vs = vt + 32 * s * V_STRIDE;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 vf = cat4(lds_tr(vs + dt * 32), lds_tr(vs + 16 * V_STRIDE + dt * 32));
        Oa[dt][0] = mfma16(vf, pb0, Oa[dt][0]);
        Oa[dt][1] = mfma16(vf, pb1, Oa[dt][1]);
      }
    }
    // lane holds O^T[d = dt*16 + 4g + r][q = qb + qt*16 + t]
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float l = sm[qt];
      l += __shfl_xor(l, 16);
      l += __shfl_xor(l, 32);
      const int q = qb + qt * 16 + t;
      if (q < L) {
        const float inv = 1.0f / l;
        uint2 x[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const f32x4 o = Oa[dt][qt];
          x[dt] = uint2{pack2bf(o[0] * inv, o[1] * inv), pack2bf(o[2] * inv, o[3] * inv)};
        }
        store_row64(O + (base + q) * ldo + h * 64, g, x);
        if (g == 0) lse[(long)nh * L + q] = mr[qt] * c + __log2f(l);
      }
    }
  }
}

// key-major (dK, dV): Q, dO, -lse, -D of every query in LDS; a wave's key chunks in turn
template <int NCH>
__global__ void __launch_bounds__(LONG_NTH)
attn_long_bwd_kv_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                        const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, long ldo,
                        const float* __restrict__ lse, bf16_t* __restrict__ dqkv, long lddq,
                        int causal, float scale) {
  constexpr int LP = 32 * NCH;
  __shared__ __attribute__((aligned(16))) char smem[2 * LP * 128 + 2 * LP * 4];
  char* Qs = smem;
  char* dOs = smem + LP * 128;
  float* nlse_s = reinterpret_cast<float*>(smem + 2 * LP * 128);  // -lse
  float* nd_s = nlse_s + LP;                                       // -D

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, t = lane & 15;
  const int nh = blockIdx.x, n = nh / H, h = nh % H;
  const long base = (long)n * L;
  const float c = scale * LOG2E;

  // staging, one pass of 512 16-B pieces at a time (three row images' registers per pass);
  // D = rowsum(dO*O) from the same chunks (8 lanes per row, reduced with xor-shuffles)
  constexpr int IT = (LP * 8 + LONG_NTH - 1) / LONG_NTH;
  const int ch = tid & 7;
#pragma unroll 2
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * LONG_NTH) >> 3;
    const long off = h * 64 + ch * 8;
    const uint4 qv = ld16_or_zero(qkv + (base + r) * ldq + off, r < L);
    const uint4 dv = ld16_or_zero(dO + (base + r) * ldo + off, r < L);
    const uint4 ov = ld16_or_zero(O + (base + r) * ldo + off, r < L);
    const float lv = (r < L) ? lse[(long)nh * L + r] : 1e30f;
    const uint32_t aa[4] = {ov.x, ov.y, ov.z, ov.w};
    const uint32_t bb[4] = {dv.x, dv.y, dv.z, dv.w};
    float dsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      dsum += bf2f(aa[k] & 0xffff) * bf2f(bb[k] & 0xffff) + bf2f(aa[k] >> 16) * bf2f(bb[k] >> 16);
    dsum = sum_row8(dsum);  // (every lane of the wave takes part: r is guarded below)
    if (r < LP) {
      *reinterpret_cast<uint4*>(Qs + r * 128 + swz(r, ch) * 16) = qv;
      *reinterpret_cast<uint4*>(dOs + r * 128 + swz(r, ch) * 16) = dv;
      if (ch == 0) {
        nd_s[r] = -dsum;
        nlse_s[r] = r < L ? -lv : -1e30f;
      }
    }
  }
  __syncthreads();

  const int ro0 = row_off(t, g, 0), ro1 = row_off(t, g, 1);
  const int tro[4] = {tr_off(t, g, 0), tr_off(t, g, 1), tr_off(t, g, 2), tr_off(t, g, 3)};

#pragma unroll 1
  for (int kc = w; kc < NCH; kc += LONG_WAVES) {  // (no barrier below)
    // own key block: K / V rows kb + kt2*16 + t, as B-operand fragments
    const int kb = 32 * kc;
    bf16x8 kf[2][2], vf[2][2];
#pragma unroll
    for (int kt2 = 0; kt2 < 2; ++kt2) {
      const int key = kb + kt2 * 16 + t;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16_t* src = qkv + (base + key) * ldq + h * 64 + s * 32 + g * 8;
        uint4 ku = ld16_or_zero(src + D, key < L), vu = ld16_or_zero(src + 2 * D, key < L);
        kf[kt2][s] = *reinterpret_cast<bf16x8*>(&ku);
        vf[kt2][s] = *reinterpret_cast<bf16x8*>(&vu);
      }
    }
    f32x4 dV[4][2], dK[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) dV[dt][k2] = dK[dt][k2] = f32x4{0.f, 0.f, 0.f, 0.f};

    // causal: queries before the block's first key see none of its keys
    const int qc0 = causal ? kc : 0;
#pragma unroll 1
    for (int qc = qc0; qc < NCH; ++qc) {
      const bool edge = (kb + 32 > L) || (causal && kb + 31 > qc * 32);
      // B operands (k = 32 queries of this chunk): slot j<4 -> q = 4g+j, j>=4 -> 16+4g+(j-4);
      // one 16-query tile of S / dP is live at a time and packed to bf16 straight away.
      u32x4 pw[2], sw[2];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int q0 = qc * 32 + qt * 16 + 4 * g;
        const f32x4 nl = *reinterpret_cast<const f32x4*>(nlse_s + q0);
        const f32x4 nd = *reinterpret_cast<const f32x4*>(nd_s + q0);
        const char* qrow = Qs + (qc * 32 + qt * 16) * 128;
        const char* drow = dOs + (qc * 32 + qt * 16) * 128;
        const bf16x8 qa0 = lds16(qrow + ro0), qa1 = lds16(qrow + ro1);
        const bf16x8 da0 = lds16(drow + ro0), da1 = lds16(drow + ro1);
        f32x4 S[2], dP[2];
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          S[k2] = mfma16(qa0, kf[k2][0], f32x4{0.f, 0.f, 0.f, 0.f});
          S[k2] = mfma16(qa1, kf[k2][1], S[k2]);
          dP[k2] = mfma16(da0, vf[k2][0], nd);  // dP - D
          dP[k2] = mfma16(da1, vf[k2][1], dP[k2]);
        }
        // lane holds X[q = q0 + r][key = kb + k2*16 + t]
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          f32x4 p;
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = ex2(__builtin_fmaf(S[k2][r], c, nl[r]));
          if (edge) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              p[r] = masked(kb + k2 * 16 + t, q0 + r, L, causal) ? 0.f : p[r];
          }
          const f32x4 ds = p * dP[k2];
          pw[k2][2 * qt] = pack2bf(p[0], p[1]);
          pw[k2][2 * qt + 1] = pack2bf(p[2], p[3]);
          sw[k2][2 * qt] = pack2bf(ds[0], ds[1]);
          sw[k2][2 * qt + 1] = pack2bf(ds[2], ds[3]);
        }
      }
      const bf16x8 pB[2] = {as_bf8(pw[0]), as_bf8(pw[1])};
      const bf16x8 sB[2] = {as_bf8(sw[0]), as_bf8(sw[1])};
      const char* qblk = Qs + qc * 32 * 128;
      const char* dblk = dOs + qc * 32 * 128;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 doT = cat4(lds_tr(dblk + tro[dt]), lds_tr(dblk + 16 * 128 + tro[dt]));
        const bf16x8 qT = cat4(lds_tr(qblk + tro[dt]), lds_tr(qblk + 16 * 128 + tro[dt]));
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          dV[dt][k2] = mfma16(doT, pB[k2], dV[dt][k2]);
          dK[dt][k2] = mfma16(qT, sB[k2], dK[dt][k2]);
        }
      }
    }
    // dK, dV of the key block: lane holds X^T[d = dt*16 + 4g + r][key = kb + k2*16 + t]
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const int key = kb + k2 * 16 + t;
      if (key < L) {
        bf16_t* dst = dqkv + (base + key) * lddq + h * 64;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const f32x4 a = dK[dt][k2], b = dV[dt][k2];
          *reinterpret_cast<uint2*>(dst + D + dt * 16 + 4 * g) =
              uint2{pack2bf(a[0] * scale, a[1] * scale), pack2bf(a[2] * scale, a[3] * scale)};
          *reinterpret_cast<uint2*>(dst + 2 * D + dt * 16 + 4 * g) =
              uint2{pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
        }
      }
    }
  }
}

// query-major (dQ): K and V of every key in LDS; a wave's query chunks in turn
template <int NCH>
__global__ void __launch_bounds__(LONG_NTH)
attn_long_bwd_q_kernel(int L, int H, int D, const bf16_t* __restrict__ qkv, long ldq,
                       const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, long ldo,
                       const float* __restrict__ lse, bf16_t* __restrict__ dqkv, long lddq,
                       int causal, float scale) {
  constexpr int LP = 32 * NCH;
  __shared__ __attribute__((aligned(16))) char smem[2 * LP * 128];
  char* Ks = smem;
  char* Vs = smem + LP * 128;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, t = lane & 15;
  // reverse order: the key-major kernel touched the last heads most recently (L2 / Infinity Cache)
  const int nh = gridDim.x - 1 - blockIdx.x, n = nh / H, h = nh % H;
  const long base = (long)n * L;
  const float c = scale * LOG2E;

  constexpr int IT = (LP * 8 + LONG_NTH - 1) / LONG_NTH;
  const int ch = tid & 7;
  uint4 kv[IT], vv[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * LONG_NTH) >> 3;
    const bf16_t* src = qkv + (base + r) * ldq + h * 64 + ch * 8;
    kv[i] = ld16_or_zero(src + D, r < L);
    vv[i] = ld16_or_zero(src + 2 * D, r < L);
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = (tid + i * LONG_NTH) >> 3;
    if (r < LP) {
      *reinterpret_cast<uint4*>(Ks + r * 128 + swz(r, ch) * 16) = kv[i];
      *reinterpret_cast<uint4*>(Vs + r * 128 + swz(r, ch) * 16) = vv[i];
    }
  }
  __syncthreads();

  const int ro0 = row_off(t, g, 0), ro1 = row_off(t, g, 1);
  const int tro[4] = {tr_off(t, g, 0), tr_off(t, g, 1), tr_off(t, g, 2), tr_off(t, g, 3)};

#pragma unroll 1
  for (int qc = w; qc < NCH; qc += LONG_WAVES) {  // (no barrier below)
    const int qb = 32 * qc;
    bf16x8 qf[2][2], df[2][2];
    float nl[2], nd[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int q = qb + qt * 16 + t;
      float dsum = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const long off = h * 64 + s * 32 + g * 8;
        uint4 u = ld16_or_zero(qkv + (base + q) * ldq + off, q < L);
        uint4 d = ld16_or_zero(dO + (base + q) * ldo + off, q < L);
        uint4 o = ld16_or_zero(O + (base + q) * ldo + off, q < L);
        qf[qt][s] = *reinterpret_cast<bf16x8*>(&u);
        df[qt][s] = *reinterpret_cast<bf16x8*>(&d);
        const uint32_t oo[4] = {o.x, o.y, o.z, o.w}, dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          dsum += bf2f(oo[k] & 0xffff) * bf2f(dd[k] & 0xffff) + bf2f(oo[k] >> 16) * bf2f(dd[k] >> 16);
      }
      dsum += __shfl_xor(dsum, 16);
      dsum += __shfl_xor(dsum, 32);
      nd[qt] = -dsum;
      nl[qt] = q < L ? -lse[(long)nh * L + q] : -1e30f;
    }
    const int s_end = causal ? min(NCH, qc + 1) : NCH;

    f32x4 dQ[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dQ[dt][0] = dQ[dt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int s = 0; s < s_end; ++s) {
      const bool edge = (32 * s + 32 > L) || (causal && 32 * s + 31 > qb);
      // one 16-key tile of S^T / dP^T live at a time, packed to bf16 straight away
      u32x4 sw[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ro = (32 * s + 16 * kk) * 128;
        const bf16x8 ka0 = lds16(Ks + ro + ro0), ka1 = lds16(Ks + ro + ro1);
        const bf16x8 va0 = lds16(Vs + ro + ro0), va1 = lds16(Vs + ro + ro1);
        f32x4 S[2], dP[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          S[qt] = mfma16(ka0, qf[qt][0], f32x4{0.f, 0.f, 0.f, 0.f});
          S[qt] = mfma16(ka1, qf[qt][1], S[qt]);
          dP[qt] = mfma16(va0, df[qt][0], f32x4{nd[qt], nd[qt], nd[qt], nd[qt]});
          dP[qt] = mfma16(va1, df[qt][1], dP[qt]);
        }
        // lane holds X^T[key = 32s + 16kk + 4g + r][q = qb + qt*16 + t]
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          f32x4 p;
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = ex2(__builtin_fmaf(S[qt][r], c, nl[qt]));
          if (edge) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              p[r] = masked(32 * s + 16 * kk + 4 * g + r, qb + qt * 16 + t, L, causal) ? 0.f : p[r];
          }
          const f32x4 ds = p * dP[qt];
          sw[qt][2 * kk] = pack2bf(ds[0], ds[1]);
          sw[qt][2 * kk + 1] = pack2bf(ds[2], ds[3]);
        }
      }
      const bf16x8 sb0 = as_bf8(sw[0]);
      const bf16x8 sb1 = as_bf8(sw[1]);
      const char* kblk = Ks + 32 * s * 128;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 kT = cat4(lds_tr(kblk + tro[dt]), lds_tr(kblk + 16 * 128 + tro[dt]));
        dQ[dt][0] = mfma16(kT, sb0, dQ[dt][0]);
        dQ[dt][1] = mfma16(kT, sb1, dQ[dt][1]);
      }
    }
    // lane holds dQ^T[d = dt*16 + 4g + r][q = qb + qt*16 + t]
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int q = qb + qt * 16 + t;
      if (q < L) {
        bf16_t* dst = dqkv + (base + q) * lddq + h * 64;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const f32x4 a = dQ[dt][qt];
          *reinterpret_cast<uint2*>(dst + dt * 16 + 4 * g) =
              uint2{pack2bf(a[0] * scale, a[1] * scale), pack2bf(a[2] * scale, a[3] * scale)};
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------- host side
// One attention launch (include/lc_clip.h has the operands' contract). The extern "C" entry
// points fill it, casts done there; check(), route() and the family launchers read it.
enum Entry { E_FWD, E_ROW_FWD, E_BWD, E_FP8, E_LIVE_ROW, E_ROW_BWD, E_LONG_FWD, E_LONG_BWD };
struct AttnArgs {
  hipStream_t stream;
  int n_seq, L, H, causal;
  const bf16_t* qkv;
  long ldq;
  const bf16_t* O;  // O and lse: the forward's outputs (its entry points take them non-const)
  long ldo;
  const float* lse;
  const bf16_t* dO = nullptr;  // from here on the backward's
  bf16_t* dqkv = nullptr;
  long lddq = 0;               // elements; bytes in the fp8 form
  int row = -1;                // the one-row forms' query row: O / dO / lse are compact then
  uint8_t* q_scale = nullptr;  // the fp8 form's E8M0 scales
  long q_rows = 0;
  int D() const { return H * 64; }
  int nqb() const { return (L + 31) / 32; }
  int items() const { return n_seq * H; }
};

constexpr float ATTN_SCALE = 0.125f;  // 64^-0.5
// 32-row chunks a kernel family takes: 8 (L <= 256), but 7 for the fused kernel's full and fp8
// modes and the two-phase kernel, which hold every chunk in LDS (BwdLds<8> does not fit, so
// attn_bwd_kernel<8> without ROW must not be instantiated)
constexpr int MAX_CHUNKS = 8, FUSED_MAX_CHUNKS = 7;
// the long family's: 257 <= L <= 512, so that every length has one home
constexpr int LONG_MIN_CHUNKS = MAX_CHUNKS + 1, LONG_MAX_CHUNKS = 16;

// 32-bit offsets. The kernels reach a sequence's rows through a raw-buffer descriptor and an int
// byte offset r * (int)ld * 2 + column bytes. r runs over the PADDED rows, up to 32 * NQB - 1
// <= 255 (attn_row_bwd_kernel: 255 whatever L is), and the column bytes end at 3 * D * 2 at the
// most (v of the last head: the k | v column offset included), within one row's bytes. So every
// offset formed, attn_row_bwd_kernel's `oob` and every descriptor's size (L rows) is at most
// 256 * row bytes. Row bytes are a multiple of 16: below 2^23 they are <= 2^23 - 16, and 256 of
// them <= 2^31 - 4096, which fits an int and stays below OOR. One bound on the strides alone
// then (ld < 2^22 elements; the fp8 form's lddq, in bytes, < 2^23), the same in all six launches.
constexpr long MAX_ROW_BYTES = 1L << 23;
static_assert(32 * MAX_CHUNKS * (MAX_ROW_BYTES - 16) < OOR && ROW_IT <= MAX_CHUNKS, "see above");
// The long family's padded rows run to 32 * LONG_MAX_CHUNKS - 1 = 511: half the stride then
// (ld < 2^21 elements), 512 * (2^22 - 16) = 2^31 - 8192.
constexpr long LONG_MAX_ROW_BYTES = 1L << 22;
static_assert(32 * LONG_MAX_CHUNKS * (LONG_MAX_ROW_BYTES - 16) < OOR, "see above");
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The one argument check: which fields entry point e has, and which limits apply to it.
int check(const AttnArgs& a, Entry e) {
  const bool lng = e == E_LONG_FWD || e == E_LONG_BWD;
  const bool fwd = e == E_FWD || e == E_ROW_FWD || e == E_LONG_FWD, fp8 = e == E_FP8;
  const bool row_pair = e == E_ROW_FWD || e == E_ROW_BWD, one_row = row_pair || e == E_LIVE_ROW;
  const int max_L = 32 * (lng ? LONG_MAX_CHUNKS : fp8 ? FUSED_MAX_CHUNKS : row_pair ? ROW_IT
                                                                          : MAX_CHUNKS);
  const int min_L = lng ? 32 * MAX_CHUNKS + 1 : 1;
  LC_CHECK_ARG(a.n_seq > 0 && a.L >= min_L && a.L <= max_L && a.H > 0);
  LC_CHECK_ARG(one_row == (a.row >= 0) && a.row < a.L);
  const long D = a.D(), es = fp8 ? 1 : 2;  // es: bytes per dqkv element
  LC_CHECK_ARG(a.ldq >= 3 * D && a.ldq % 8 == 0 && a.ldo >= D && a.ldo % 8 == 0);
  // rows moved as 16-B pieces by pointer: the forward's O, the compact O / dO rows, dqkv
  LC_CHECK_ARG(!(fwd || one_row) || aligned16(a.O));
  if (!fwd) {
    LC_CHECK_ARG(!one_row || aligned16(a.dO));
    LC_CHECK_ARG(a.lddq >= 3 * D && a.lddq % (16 / es) == 0 && aligned16(a.dqkv));
  }
  if (fp8)
    LC_CHECK_ARG(a.q_scale != nullptr && a.q_rows % 256 == 0 &&
                 a.q_rows >= ((long)a.n_seq * a.L + 255) / 256 * 256);
  const long max_rb = lng ? LONG_MAX_ROW_BYTES : MAX_ROW_BYTES;
  LC_CHECK_ARG(a.ldq < max_rb / 2 && a.ldo < max_rb / 2 && a.lddq < max_rb / es);
  return LC_OK;
}

// lc_attn_bwd_set_form: 0 automatic, else one of these
enum { ATTN_BWD_FUSED = 1, ATTN_BWD_SPLIT = 2, ATTN_BWD_TWO_PHASE = 3 };
const int g_att2_ko = [] {  // DIAG builds: attn_bwd2_kernel timing knockouts
  const char* e = lc_diag_env("LC_ATT2_KO");
  return e ? atoi(e) : 0;
}();
int g_attn_bwd_form = [] {  // DIAG builds: LC_ATTN_BWD_FORM=<form>, LC_ATTN_BWD_SPLIT=1 (A/Bs)
  const char* f = lc_diag_env("LC_ATTN_BWD_FORM");
  if (f) return atoi(f);
  const char* e = lc_diag_env("LC_ATTN_BWD_SPLIT");
  return e && atoi(e) ? (int)ATTN_BWD_SPLIT : 0;
}();
const bool g_fwd_online = [] {  // DIAG builds: LCCLIP_ATTN_FWD_ONLINE=0: the two-pass forward
  const char* e = lc_diag_env("LCCLIP_ATTN_FWD_ONLINE");
  return !(e && e[0] == '0');
}();

// The kernel family a checked launch runs on, decided here and nowhere else (table: DESIGN.md).
enum Family { F_REFUSE, F_FORWARD, F_FUSED, F_SPLIT, F_TWO_PHASE, F_ROW_VALU, F_LONG };
Family route(Entry e, int nqb, int form) {
  switch (e) {
    case E_FWD: case E_ROW_FWD: return F_FORWARD;
    case E_ROW_BWD: return F_ROW_VALU;
    // 9..16 chunks: one form, whatever lc_attn_bwd_set_form says
    case E_LONG_FWD: case E_LONG_BWD: return F_LONG;
    case E_FP8: return F_FUSED;
    // the result is the default form's (fused kernel; key-major + query-major pair at 8 chunks)
    case E_LIVE_ROW: return form == 0 || form == ATTN_BWD_FUSED ? F_FUSED : F_REFUSE;
    case E_BWD: break;
  }
  // fused single-pass kernel (dS^T parked in LDS, 1 workgroup per CU) up to 224 keys; the split
  // key-major + query-major pair beyond that (LDS); lc_attn_bwd_set_form selects another form
  if (nqb > FUSED_MAX_CHUNKS || form == ATTN_BWD_SPLIT) return F_SPLIT;
  return form == ATTN_BWD_TWO_PHASE ? F_TWO_PHASE : F_FUSED;
}

// f(std::integral_constant<int, nqb>) for nqb in MIN..MAX (the family's chunk limits: nothing
// outside them is instantiated), LC_EINVAL outside; f(std::true_type / std::false_type) for a flag
template <int MAX, int MIN = 1, class F>
int with_chunks(int nqb, const F& f) {
  if constexpr (MAX < MIN) return LC_EINVAL;
  else return nqb == MAX ? f(std::integral_constant<int, MAX>{}) : with_chunks<MAX - 1, MIN>(nqb, f);
}
template <class F>
int with_flag(bool flag, const F& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// workgroups of a persistent launch: as many as fit on the chip at once (LDS-limited) when there
// are many items per workgroup (L = 197: 3072 items, 12 per workgroup), else one per item
int persistent_grid(int items, int lds_bytes) {
  int per_cu = (160 * 1024) / lds_bytes;
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  const int g = cu_count() * per_cu;
  // a few items per workgroup would leave a ragged last round: one item each (no pipelining)
  return items < 4 * g ? items : g;
}

int launch_fwd(const AttnArgs& a) {
  return with_chunks<MAX_CHUNKS>(a.nqb(), [&](auto Q) {
    return with_flag(g_fwd_online, [&](auto ONLINE) {
      return with_flag(a.row >= 0, [&](auto ROW) -> int {
        constexpr int NQB = decltype(Q)::value;
        hipLaunchKernelGGL((attn_fwd_kernel<NQB, decltype(ONLINE)::value, decltype(ROW)::value>),
                           dim3(a.items()), dim3(64 * NQB), 0, a.stream, a.L, a.H, a.D(), a.qkv,
                           a.ldq, const_cast<bf16_t*>(a.O), a.ldo, const_cast<float*>(a.lse),
                           a.causal, ATTN_SCALE, a.row >= 0 ? a.row : 0);
        LC_LAUNCH_RET();
      });
    });
  });
}

// full (Q8 = ROW = false), fp8 outputs (Q8) or the one-row mode (ROW: q_rows carries the row).
// The grid rule, once: persistent from 5 chunks (the kernel's PERSIST), else a workgroup per item.
template <bool Q8, bool ROW>
int launch_fused(const AttnArgs& a) {
  return with_chunks<ROW ? MAX_CHUNKS : FUSED_MAX_CHUNKS>(a.nqb(), [&](auto Q) -> int {
    constexpr int NQB = decltype(Q)::value;
    using Lay = typename std::conditional<ROW, BwdLdsRow<NQB>, BwdLds<NQB>>::type;
    const int grid = NQB >= 5 ? persistent_grid(a.items(), Lay::BYTES) : a.items();
    hipLaunchKernelGGL((attn_bwd_kernel<NQB, (NQB >= 5), Q8, ROW>), dim3(grid), dim3(64 * NQB), 0,
                       a.stream, a.items(), a.L, a.H, a.D(), a.qkv, a.ldq, a.O, a.dO, a.ldo, a.lse,
                       a.dqkv, a.lddq, a.causal, ATTN_SCALE, a.q_scale,
                       ROW ? (long)a.row : a.q_rows);
    LC_LAUNCH_RET();
  });
}

int launch_split(const AttnArgs& a) {  // key-major (dK, dV), then query-major (dQ)
  return with_chunks<MAX_CHUNKS>(a.nqb(), [&](auto Q) -> int {
    constexpr int NQB = decltype(Q)::value;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(a.items()), dim3(64 * NQB), 0, a.stream, a.L, a.H, a.D(),
                         a.qkv, a.ldq, a.O, a.dO, a.ldo, a.lse, a.dqkv, a.lddq, a.causal,
                         ATTN_SCALE);
    };
    launch(attn_bwd_kv_kernel<NQB>);
    launch(attn_bwd_q_kernel<NQB>);
    LC_LAUNCH_RET();
  });
}

int launch_two_phase(const AttnArgs& a) {
  return with_chunks<FUSED_MAX_CHUNKS>(a.nqb(), [&](auto Q) {
    return with_flag(a.causal != 0, [&](auto CAUSAL) -> int {
      constexpr int NQB = decltype(Q)::value;
      hipLaunchKernelGGL((attn_bwd2_kernel<NQB, decltype(CAUSAL)::value>), dim3(a.items()),
                         dim3(64 * NQB), 0, a.stream, a.L, a.H, a.D(), a.qkv, a.ldq, a.O, a.dO,
                         a.ldo, a.lse, a.dqkv, a.lddq, ATTN_SCALE, g_att2_ko);
      LC_LAUNCH_RET();
    });
  });
}

int launch_row_valu(const AttnArgs& a) {
  hipLaunchKernelGGL(attn_row_bwd_kernel, dim3(a.items()), dim3(ROW_NTH), 0, a.stream, a.L, a.H,
                     a.D(), a.qkv, a.ldq, a.row, a.O, a.dO, a.ldo, a.lse, a.dqkv, a.lddq, a.causal,
                     ATTN_SCALE);
  LC_LAUNCH_RET();
}

// the long family: the forward, or the key-major (dK, dV) then the query-major (dQ) kernel
int launch_long(Entry e, const AttnArgs& a) {
  return with_chunks<LONG_MAX_CHUNKS, LONG_MIN_CHUNKS>(a.nqb(), [&](auto Q) -> int {
    constexpr int NCH = decltype(Q)::value;
    if (e == E_LONG_FWD) {
      hipLaunchKernelGGL(attn_long_fwd_kernel<NCH>, dim3(a.items()), dim3(LONG_NTH), 0, a.stream,
                         a.L, a.H, a.D(), a.qkv, a.ldq, const_cast<bf16_t*>(a.O), a.ldo,
                         const_cast<float*>(a.lse), a.causal, ATTN_SCALE);
      LC_LAUNCH_RET();
    }
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(a.items()), dim3(LONG_NTH), 0, a.stream, a.L, a.H, a.D(),
                         a.qkv, a.ldq, a.O, a.dO, a.ldo, a.lse, a.dqkv, a.lddq, a.causal,
                         ATTN_SCALE);
    };
    launch(attn_long_bwd_kv_kernel<NCH>);
    launch(attn_long_bwd_q_kernel<NCH>);
    LC_LAUNCH_RET();
  });
}

// Every launching entry point: check, route, launch on the family the route names.
int run(Entry e, const AttnArgs& a) {
  if (const int rc = check(a, e)) return rc;
  switch (route(e, a.nqb(), g_attn_bwd_form)) {
    case F_FORWARD: return launch_fwd(a);
    case F_FUSED:
      return a.q_scale   ? launch_fused<true, false>(a)
             : a.row >= 0 ? launch_fused<false, true>(a) : launch_fused<false, false>(a);
    case F_SPLIT: return launch_split(a);
    case F_TWO_PHASE: return launch_two_phase(a);
    case F_ROW_VALU: return launch_row_valu(a);
    case F_LONG: return launch_long(e, a);
    case F_REFUSE: break;
  }
  return LC_EUNSUPPORTED;
}

}  // namespace

extern "C" {

int lc_attn_fwd(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq, void* O,
                long ldo, float* lse, int causal) {
  return run(E_FWD, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O, ldo,
                     lse});
}

int lc_attn_bwd_fp8(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq,
                    const void* O, const void* dO, long ldo, const float* lse, void* dqkv, long lddq,
                    void* q_scale, long q_rows, int causal) {
  return run(E_FP8, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O, ldo, lse,
                     (const bf16_t*)dO, (bf16_t*)dqkv, lddq, -1, (uint8_t*)q_scale, q_rows});
}

int lc_attn_bwd_set_form(int form) {
  if (form < 0 || form > ATTN_BWD_TWO_PHASE) return LC_EINVAL;
  g_attn_bwd_form = form;
  return LC_OK;
}

int lc_attn_bwd(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq, const void* O,
                const void* dO, long ldo, const float* lse, void* dqkv, long lddq, int causal) {
  return run(E_BWD, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O, ldo, lse,
                     (const bf16_t*)dO, (bf16_t*)dqkv, lddq});
}

int lc_attn_long_fwd(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq, void* O,
                     long ldo, float* lse, int causal) {
  return run(E_LONG_FWD, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O, ldo,
                          lse});
}

int lc_attn_long_bwd(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq,
                     const void* O, const void* dO, long ldo, const float* lse, void* dqkv,
                     long lddq, int causal) {
  return run(E_LONG_BWD, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O, ldo,
                          lse, (const bf16_t*)dO, (bf16_t*)dqkv, lddq});
}

int lc_attn_bwd_live_row(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq,
                         int row, const void* O_row, const void* dO_row, long ldo,
                         const float* lse_row, void* dqkv, long lddq, int causal) {
  return run(E_LIVE_ROW, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O_row,
                          ldo, lse_row, (const bf16_t*)dO_row, (bf16_t*)dqkv, lddq, row});
}

int lc_attn_row_fwd(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq, int row,
                    void* O_row, long ldo, float* lse_row, int causal) {
  return run(E_ROW_FWD, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O_row,
                         ldo, lse_row, nullptr, nullptr, 0, row});
}

int lc_attn_row_bwd(hipStream_t st, int n_seq, int L, int H, const void* qkv, long ldq, int row,
                    const void* O_row, const void* dO_row, long ldo, const float* lse_row,
                    void* dqkv, long lddq, int causal) {
  return run(E_ROW_BWD, {st, n_seq, L, H, causal, (const bf16_t*)qkv, ldq, (const bf16_t*)O_row,
                         ldo, lse_row, (const bf16_t*)dO_row, (bf16_t*)dqkv, lddq, row});
}

}  // extern "C"

