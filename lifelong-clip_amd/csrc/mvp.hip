// MVP-CLIP (BASELINE config 3) training method: the prompt-pool glue and the scored loss.
//   models/mvp_clip.py:224-235, 253   key distance, top-k selection, count       (lc_mvp_select)
//   models/mvp_clip.py:239-248        similarity loss, plain and contrastive     (lc_mvp_simloss*)
//   models/mvp_clip.py:236-237        e_prompts[topk], mask[topk].mean(1)        (lc_pool_gather*)
//   methods/mvp_clip.py:265-276       masked logits + exposed-class mask + NLL   (lc_mvp_head_fwd)
//   methods/mvp_clip.py:204-254       ign / cps scores, the loop of B backward passes in closed
//                                     form                                       (lc_mvp_score*)
//   methods/mvp_clip.py:277-280       the GSF loss weight                        (lc_mvp_loss_mean)
// Everything is f32 in, f32 out, wave64. Every reduction runs in a fixed order (per-thread
// strided partial, xor butterfly, waves in index order), and no floating-point atomic is used,
// so two launches on the same inputs are bit-identical. The only atomics are the integer
// selection counts.
#include "lc_common.h"

namespace {

constexpr float COS_EPS = 1e-8f;  // torch.cosine_similarity: each norm clamped at eps
constexpr int MVP_MAXW = 4096;    // query / key width held in LDS
constexpr int MVP_MAXP = 64;      // pool entries (one wave holds one candidate each)

// sum over the 256 threads of a workgroup, the four waves' partials added in wave order
LC_DEV float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

LC_DEV float sigmoid2(float x) { return 2.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------- selection
// one workgroup per image row: the query row in LDS, waves over pool entries, wave 0 runs the k
// argmin rounds (lane p holds entry p; ties go to the lower index)
__global__ void __launch_bounds__(256)
mvp_select_kernel(int B, int P, int W, int K, const float* __restrict__ query, long ldq,
                  const float* __restrict__ key, long ldk, const float* __restrict__ count,
                  int64_t* __restrict__ idx, float* __restrict__ dist, float* __restrict__ qn,
                  float* __restrict__ kn, unsigned long long* __restrict__ hist) {
  __shared__ float qrow[MVP_MAXW];
  __shared__ float red[4];
  __shared__ float d_s[MVP_MAXP], sd_s[MVP_MAXP];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float ss = 0.f;
  for (int k = tid; k < W; k += 256) {
    const float v = query[(long)b * ldq + k];
    qrow[k] = v;
    ss += v * v;
  }
  const float qnorm = fmaxf(sqrtf(block_sum256(ss, red)), COS_EPS);
  for (int p = w; p < P; p += 4) {
    float dot = 0.f, kk = 0.f;
    for (int k = lane; k < W; k += 64) {
      const float v = key[(long)p * ldk + k];
      dot += qrow[k] * v;
      kk += v * v;
    }
    dot = wave_sum(dot);
    kk = wave_sum(kk);
    if (lane == 0) {
      const float knorm = fmaxf(sqrtf(kk), COS_EPS);
      const float d = 1.0f - dot / (qnorm * knorm);
      d_s[p] = d;
      sd_s[p] = count ? d * (count[p] + 1.0f) : d;
      if (b == 0) kn[p] = knorm;
    }
  }
  __syncthreads();
  if (w != 0) return;
  if (lane == 0) qn[b] = qnorm;
  // a candidate is (value, index); lanes without a live entry carry (+inf, 64 + lane), which
  // loses every tie against a live one, so the winner always indexes the pool (K <= P)
  float v = lane < P ? sd_s[lane] : INFINITY;
  if (!(v == v)) v = INFINITY;
  int i = lane < P ? lane : 64 + lane;
  for (int r = 0; r < K; ++r) {
    float bv = v;
    int bi = i;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (lane == 0) {
      idx[(long)b * K + r] = bi;
      dist[(long)b * K + r] = d_s[bi];
      if (hist) atomicAdd(&hist[bi], 1ull);
    }
    if (lane == bi) v = INFINITY, i = 64 + lane;
  }
}

// kcos[i][j] = cos(key_i, key_j) with the clamped norms of the selection kernel
__global__ void __launch_bounds__(256)
mvp_keycos_kernel(int P, int W, const float* __restrict__ key, long ldk,
                  const float* __restrict__ kn, float* __restrict__ kcos) {
  __shared__ float krow[MVP_MAXW];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int k = tid; k < W; k += 256) krow[k] = key[(long)i * ldk + k];
  __syncthreads();
  for (int j = w; j < P; j += 4) {
    float dot = 0.f;
    for (int k = lane; k < W; k += 64) dot += krow[k] * key[(long)j * ldk + k];
    dot = wave_sum(dot);
    if (lane == 0) kcos[i * P + j] = dot / (kn[i] * kn[j]);
  }
}

// ---------------------------------------------------------------- similarity loss
// One workgroup. Plain: loss = mean of the selected distances. Contrastive (selection size 1,
// the only size at which the reference's expression broadcasts for a general batch): with
// t_b = idx[b], mass = count + 1, h[p] = #{b: t_b = p},
//   A = mean_{a,b,p} exp(kwd[t_a][p] / mass[t_b]),  D = mean_{a,b} exp(dist[b] / mass[t_a])
//   loss = -log(A / (D + A) + 1e-6)
// (key_wise_distance[topk] is [B,1,P] and mass[topk] is [B,1]: their quotient broadcasts to
// [B,B,P]; distance is [B] after the squeeze and its quotient [B,B].)
// rawgd[n] and rawW[i][p] are d(sum)/d(dist[n]) and d(sum)/d(kwd[i][p]); coef = {dloss/dD-sum,
// dloss/dA-sum} turns them into loss gradients in the backward kernel.
__global__ void __launch_bounds__(256)
mvp_simloss_kernel(int B, int P, int K, int contrastiv, const float* __restrict__ count,
                   const int64_t* __restrict__ idx, const float* __restrict__ dist,
                   const float* __restrict__ kcos, float* __restrict__ rawgd,
                   float* __restrict__ rawW, float* __restrict__ coef, float* __restrict__ loss) {
  __shared__ float red[4];
  __shared__ float h[MVP_MAXP], im[MVP_MAXP];
  const int tid = threadIdx.x;
  const int N = B * K;
  if (!contrastiv) {
    float s = 0.f;
    for (int n = tid; n < N; n += 256) {
      s += dist[n];
      rawgd[n] = 1.0f;
    }
    const float tot = block_sum256(s, red);
    if (tid == 0) {
      loss[0] = tot / (float)N;
      coef[0] = 1.0f / (float)N;
      coef[1] = 0.f;
    }
    return;
  }
  if (tid < MVP_MAXP) {
    int c = 0;
    if (tid < P)
      for (int n = 0; n < N; ++n) c += idx[n] == tid;
    h[tid] = (float)c;
    im[tid] = tid < P ? 1.0f / (count[tid] + 1.0f) : 0.f;
  }
  __syncthreads();
  float a = 0.f;
  for (int it = tid; it < P * P; it += 256) {
    const int i = it / P;
    const float kwd = 1.0f - kcos[it];
    float e = 0.f, ew = 0.f;
    for (int j = 0; j < P; ++j)
      if (h[j] > 0.f) {
        const float t = h[j] * expf(kwd * im[j]);
        e += t;
        ew += t * im[j];
      }
    a += h[i] * e;
    rawW[it] = h[i] * ew;
  }
  float d = 0.f;
  for (int n = tid; n < N; n += 256) {
    const float dn = dist[n];
    float e = 0.f, ew = 0.f;
    for (int j = 0; j < P; ++j)
      if (h[j] > 0.f) {
        const float t = h[j] * expf(dn * im[j]);
        e += t;
        ew += t * im[j];
      }
    d += e;
    rawgd[n] = ew;
  }
  const float nA = (float)B * (float)B * (float)P, nD = (float)B * (float)B;
  const float A = block_sum256(a, red) / nA;
  const float D = block_sum256(d, red) / nD;
  if (tid == 0) {
    const float r = A / (D + A);
    loss[0] = -logf(r + 1e-6f);
    const float g = -1.0f / (r + 1e-6f);
    const float den = (D + A) * (D + A);
    coef[0] = -g * A / den / nD;  // dloss/dD / (B B)
    coef[1] = g * D / den / nA;   // dloss/dA / (B B P)
  }
}

// dkey[p], one workgroup per pool entry: its (b, s) contributors in ascending order, then (the
// contrastive form) the other keys in index order. d(1 - cos(u, v))/dv = -(u/|u| - cos v/|v|)/|v|.
__global__ void __launch_bounds__(256)
mvp_simloss_bwd_kernel(int B, int P, int W, int K, int contrastiv,
                       const float* __restrict__ query, long ldq, const float* __restrict__ key,
                       long ldk, const int64_t* __restrict__ idx, const float* __restrict__ dist,
                       const float* __restrict__ qn, const float* __restrict__ kn,
                       const float* __restrict__ kcos, const float* __restrict__ rawgd,
                       const float* __restrict__ rawW, const float* __restrict__ coef,
                       const float* __restrict__ up, float* __restrict__ dkey, long ldd) {
  // The entry's contributors are first compacted, in ascending order, into LDS by wave 0
  // (coalesced reads of idx, ballot + prefix count), 1024 positions at a time; the column loop
  // then streams their query rows with independent loads. (Walking idx inside the column loop
  // made every contributor a chain of dependent scalar loads: 200 us at B = 128.)
  __shared__ int hit_b[1024];
  __shared__ float hit_a[1024];
  __shared__ int nhit_s;
  __shared__ float csum_s;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int N = B * K;
  const float u = up ? up[0] : 1.0f;
  const float cD = coef[0] * u, cA = coef[1] * u;
  const float inv_kp = 1.0f / kn[p];
  for (int n0 = 0; n0 < N; n0 += 1024) {
    __syncthreads();
    if (tid < 64) {
      int base = 0;
      float cs = 0.f;
      for (int j = 0; j < 16; ++j) {
        const int n = n0 + j * 64 + lane;
        const bool hit = n < N && idx[n] == p;
        const unsigned long long m = __ballot(hit);
        float v = 0.f;
        if (hit) {
          const int b = n / K;
          const float g = cD * rawgd[n];
          const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
          hit_b[pos] = b;
          hit_a[pos] = g / qn[b];
          v = g * (1.0f - dist[n]);
        }
        cs += wave_sum(v);
        base += __popcll(m);
      }
      if (lane == 0) nhit_s = base, csum_s = cs;
    }
    __syncthreads();
    const int nhit = nhit_s;
    const float csum = csum_s;  // sum_hits g cos(q_b, key_p)
    for (int w = tid; w < W; w += 256) {
      const float kpw = key[(long)p * ldk + w] * inv_kp;
      float a = 0.f;  // sum_hits (g / |q_b|) q[b][w]
#pragma unroll 4
      for (int t = 0; t < nhit; ++t) a += hit_a[t] * query[(long)hit_b[t] * ldq + w];
      float r = -(a - csum * kpw) * inv_kp;
      if (n0 == 0) {
        if (contrastiv) {
          for (int i = 0; i < P; ++i) {
            const float ws = cA * (rawW[i * P + p] + rawW[p * P + i]);
            if (ws == 0.f) continue;
            r -= ws * (key[(long)i * ldk + w] / kn[i] - kcos[i * P + p] * kpw) * inv_kp;
          }
        }
        dkey[(long)p * ldd + w] = r;
      } else {
        dkey[(long)p * ldd + w] += r;  // later chunks of 1024 positions: the same thread, in order
      }
    }
  }
}

// ---------------------------------------------------------------- pool gather
// out[n] = table[idx[n]] (mean = 0, n over B K rows) or out[b] = mean_s table[idx[b][s]]
// (mean = 1). An index outside the pool gives a NaN row.
template <bool V4>
__global__ void __launch_bounds__(256)
mvp_gather_kernel(int K, int P, long R, const float* __restrict__ table, long ldt,
                  const int64_t* __restrict__ idx, float* __restrict__ out, int mean) {
  const long row = blockIdx.y;
  const long col = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (col >= R) return;
  const int ns = mean ? K : 1;
  const float sc = mean ? 1.0f / (float)K : 1.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < ns; ++s) {
    const int64_t e = idx[row * ns + s];
    float4 v;
    if (e < 0 || e >= P) {
      v.x = v.y = v.z = v.w = __builtin_nanf("");
    } else if (V4) {
      v = *reinterpret_cast<const float4*>(table + e * ldt + col);
    } else {
      const float* t = table + e * ldt + col;
      v.x = t[0];
      v.y = col + 1 < R ? t[1] : 0.f;
      v.z = col + 2 < R ? t[2] : 0.f;
      v.w = col + 3 < R ? t[3] : 0.f;
    }
    acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
  }
  if (mean) acc.x *= sc, acc.y *= sc, acc.z *= sc, acc.w *= sc;
  float* o = out + row * R + col;
  if (V4) {
    *reinterpret_cast<float4*>(o) = acc;
  } else {
    o[0] = acc.x;
    if (col + 1 < R) o[1] = acc.y;
    if (col + 2 < R) o[2] = acc.z;
    if (col + 3 < R) o[3] = acc.w;
  }
}

// counting sort of idx[N] by pool entry: ws[0..P] = offsets, ws[P+1 ..] = the positions n of
// each entry in ascending order (indices outside the pool are left out)
__global__ void __launch_bounds__(128)
mvp_sort_kernel(int N, int P, const int64_t* __restrict__ idx, int* __restrict__ ws) {
  __shared__ int cnt[MVP_MAXP];
  __shared__ int off[MVP_MAXP + 1];
  const int tid = threadIdx.x;
  if (tid < MVP_MAXP) {
    int c = 0;
    if (tid < P)
      for (int n = 0; n < N; ++n) c += idx[n] == tid;
    cnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    off[0] = 0;
    for (int j = 0; j < P; ++j) off[j + 1] = off[j] + cnt[j];
  }
  __syncthreads();
  if (tid <= P) ws[tid] = off[tid];
  if (tid < P) {
    int o = off[tid];
    for (int n = 0; n < N; ++n)
      if (idx[n] == tid) ws[P + 1 + o++] = n;
  }
}

// dtable[p] = alpha * sum of the gradient rows of entry p's contributors, in ascending (b, s)
// order; one wave per (entry, 256-column chunk), 16-B loads, several rows in flight
template <bool V4>
__global__ void __launch_bounds__(64)
mvp_gather_bwd_kernel(int K, int P, long R, const int* __restrict__ ws,
                      const float* __restrict__ g, long ldg, int shared_s, float alpha,
                      float* __restrict__ dtable, long ldd) {
  const int p = blockIdx.y;
  const long col = ((long)blockIdx.x * 64 + threadIdx.x) * 4;
  if (col >= R) return;
  const int lo = ws[p], hi = ws[p + 1];
  const int* perm = ws + P + 1;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int t = lo; t < hi; ++t) {
    const int n = perm[t];
    const float* src = g + (long)(shared_s ? n / K : n) * ldg + col;
    float4 v;
    if (V4) {
      v = *reinterpret_cast<const float4*>(src);
    } else {
      v.x = src[0];
      v.y = col + 1 < R ? src[1] : 0.f;
      v.z = col + 2 < R ? src[2] : 0.f;
      v.w = col + 3 < R ? src[3] : 0.f;
    }
    acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
  }
  acc.x *= alpha, acc.y *= alpha, acc.z *= alpha, acc.w *= alpha;
  float* o = dtable + (long)p * ldd + col;
  if (V4) {
    *reinterpret_cast<float4*>(o) = acc;
  } else {
    o[0] = acc.x;
    if (col + 1 < R) o[1] = acc.y;
    if (col + 2 < R) o[2] = acc.z;
    if (col + 3 < R) o[3] = acc.w;
  }
}

// ---------------------------------------------------------------- head
// one workgroup per image row: u = s cos (the unmasked logits), z = u m + cmask,
// p = softmax(z), nll = -log p[y], q1 = 1 - p[y] as sum_{c != y} e_c / Z
__global__ void __launch_bounds__(256)
mvp_head_fwd_kernel(int B, int C, int E, const float* __restrict__ img_n,
                    const float* __restrict__ txt_n, const float* __restrict__ logit_scale,
                    const float* __restrict__ maskrows, long ldm, const float* __restrict__ cmask,
                    const int64_t* __restrict__ labels, float* __restrict__ logits,
                    float* __restrict__ u, float* __restrict__ probs, float* __restrict__ nll,
                    float* __restrict__ q1) {
  __shared__ float irow[1024];
  __shared__ float zs[1024];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float s = expf(*logit_scale);
  for (int k = tid; k < E; k += 256) irow[k] = img_n[(long)b * E + k];
  __syncthreads();
  for (int c = w; c < C; c += 4) {
    float d = 0.f;
    for (int k = lane; k < E; k += 64) d += irow[k] * txt_n[(long)c * E + k];
    d = wave_sum(d);
    if (lane == 0) {
      const float uu = s * d;
      const float m = maskrows ? sigmoid2(maskrows[(long)b * ldm + c]) : 1.0f;
      const float z = uu * m + (cmask ? cmask[c] : 0.f);
      u[(long)b * C + c] = uu;
      zs[c] = z;
      logits[(long)b * C + c] = z;
    }
  }
  __syncthreads();
  if (w != 0) return;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, zs[c]);
  mx = wave_max(mx);
  const int64_t y64 = labels[b];
  const bool valid = y64 >= 0 && y64 < C;
  const int y = valid ? (int)y64 : -1;
  float Z = 0.f, other = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float e = expf(zs[c] - mx);
    Z += e;
    if (c != y) other += e;
  }
  Z = wave_sum(Z);
  other = wave_sum(other);
  for (int c = lane; c < C; c += 64) probs[(long)b * C + c] = expf(zs[c] - mx) / Z;
  if (lane == 0) {
    // a label outside [0, C) or on an unexposed (-inf) column poisons the loss and, through a
    // NaN q1, this row's gradients and scores, so the non-finite check skips the update
    // (lc_clip_head does the same)
    nll[b] = valid ? (mx - zs[y]) + logf(Z) : __builtin_nanf("");
    q1[b] = valid && zs[y] != -INFINITY ? other / Z : __builtin_nanf("");
  }
}

// lbar = mean nll (fixed order); w = (1 - alpha) + alpha * gsf_sum / n_global (1 without GSF);
// loss = lbar * w
__global__ void __launch_bounds__(256)
mvp_loss_mean_kernel(int B, const float* __restrict__ nll, const float* __restrict__ gsf_sum,
                     float alpha, float inv_n, float* __restrict__ loss, float* __restrict__ wout,
                     float* __restrict__ lbar) {
  __shared__ float red[4];
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) s += nll[b];
  const float tot = block_sum256(s, red);
  if (threadIdx.x == 0) {
    const float L = tot / (float)B;
    const float w = gsf_sum ? (1.0f - alpha) + alpha * gsf_sum[0] * inv_n : 1.0f;
    loss[0] = L * w;
    wout[0] = w;
    lbar[0] = L;
  }
}

// G[c] = scale * s * sum_b m[b][c] (p[b][c] - [y_b == c]) img_n[b], one workgroup per class
// walking the batch in order (the head_feat_grad pattern: thread t owns columns t + 256 j)
__global__ void __launch_bounds__(256)
mvp_score_g_kernel(int B, int C, int E, const float* __restrict__ img_n,
                   const float* __restrict__ probs, const float* __restrict__ q1,
                   const float* __restrict__ maskrows, long ldm,
                   const float* __restrict__ logit_scale, const int64_t* __restrict__ labels,
                   float scale, float* __restrict__ G) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const float s = expf(*logit_scale) * scale;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    const float pm = labels[b] == c ? -q1[b] : probs[(long)b * C + c];
    const float m = maskrows ? sigmoid2(maskrows[(long)b * ldm + c]) : 1.0f;
    const float coef = m * pm;
    if (coef == 0.f) continue;
    const float* row = img_n + (long)b * E;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (tid + 256 * j < E) acc[j] += coef * row[tid + 256 * j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (tid + 256 * j < E) G[(long)c * E + tid + 256 * j] = acc[j] * s;
}

// ign[b] = 1 - cos(sample_grad_b, G[y_b]), sample_grad_b = s m[b][y] (p[b][y] - 1) img_n[b];
// cps[b] = 1 - cos(txt[y_b], img[b]) + margin. One wave per row.
__global__ void __launch_bounds__(64)
mvp_score_rows_kernel(int B, int C, int E, const float* __restrict__ img_n,
                      const float* __restrict__ txt_n, const float* __restrict__ G,
                      const float* __restrict__ q1, const float* __restrict__ maskrows, long ldm,
                      const float* __restrict__ logit_scale, const int64_t* __restrict__ labels,
                      float margin, float* __restrict__ ign, float* __restrict__ cps) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t y = labels[b];
  if (y < 0 || y >= C) {
    if (lane == 0) ign[b] = cps[b] = __builtin_nanf("");
    return;
  }
  const float m = maskrows ? sigmoid2(maskrows[(long)b * ldm + y]) : 1.0f;
  const float a = expf(*logit_scale) * m * -q1[b];
  float sb = 0.f, ss = 0.f, bb = 0.f, ti = 0.f, tt = 0.f, ii = 0.f;
  for (int k = lane; k < E; k += 64) {
    const float iv = img_n[(long)b * E + k], gv = G[y * E + k], tv = txt_n[y * E + k];
    const float sg = a * iv;
    sb += sg * gv, ss += sg * sg, bb += gv * gv;
    ti += tv * iv, tt += tv * tv, ii += iv * iv;
  }
  sb = wave_sum(sb), ss = wave_sum(ss), bb = wave_sum(bb);
  ti = wave_sum(ti), tt = wave_sum(tt), ii = wave_sum(ii);
  if (lane == 0) {
    ign[b] = 1.0f - sb / (fmaxf(sqrtf(ss), COS_EPS) * fmaxf(sqrtf(bb), COS_EPS));
    cps[b] = 1.0f - ti / (fmaxf(sqrtf(tt), COS_EPS) * fmaxf(sqrtf(ii), COS_EPS)) + margin;
  }
}

// out[0] = sum_b ign[b]^gamma, fixed order
__global__ void __launch_bounds__(256)
mvp_ign_sum_kernel(int B, const float* __restrict__ ign, float gamma, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) s += powf(ign[b], gamma);
  const float tot = block_sum256(s, red);
  if (threadIdx.x == 0) out[0] = tot;
}

// AFS (methods/mvp_clip.py:264-266): the feature divided by cps, then normalised, is
// sign(cps) n with norm |f| / |cps|; the chain through the division makes the effective
// divisor of lc_head_feat_grad sign(cps) |f|. cps == 0 gives NaN, as 0/0 does there.
__global__ void __launch_bounds__(64)
mvp_afs_kernel(int B, int E, const float* __restrict__ img_n, const float* __restrict__ norms,
               const float* __restrict__ cps, float* __restrict__ out_n,
               float* __restrict__ out_norms) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float c = cps[b];
  const float sg = c > 0.f ? 1.0f : (c < 0.f ? -1.0f : __builtin_nanf(""));
  for (int k = lane; k < E; k += 64) out_n[(long)b * E + k] = img_n[(long)b * E + k] * sg;
  if (lane == 0) out_norms[b] = norms[b] * sg;
}

// dz = w (p - onehot) / B; dlog = dz m (to the unmasked logits u), dmask = dz u m' (to the
// pre-sigmoid mask row; columns C .. NC-1 of the row get 0)
__global__ void __launch_bounds__(256)
mvp_head_bwd_kernel(int B, int C, int NC, const float* __restrict__ probs,
                    const float* __restrict__ q1, const float* __restrict__ u,
                    const float* __restrict__ maskrows, long ldm,
                    const int64_t* __restrict__ labels, const float* __restrict__ wdev,
                    float inv_b, float* __restrict__ dlog, float* __restrict__ dmask, long ldd) {
  const int b = blockIdx.x;
  const int64_t y = labels[b];
  const bool valid = y >= 0 && y < C;
  const float w = (wdev ? wdev[0] : 1.0f) * inv_b;
  const int n = dmask ? NC : C;
  for (int c = threadIdx.x; c < n; c += 256) {
    if (c >= C) {
      dmask[(long)b * ldd + c] = 0.f;
      continue;
    }
    float dz = w * (c == y ? -q1[b] : probs[(long)b * C + c]);
    if (!valid || q1[b] != q1[b]) dz = __builtin_nanf("");
    float m = 1.0f;
    if (maskrows) {
      const float sg = 1.0f / (1.0f + expf(-maskrows[(long)b * ldm + c]));
      m = 2.0f * sg;
      if (dmask) dmask[(long)b * ldd + c] = dz * u[(long)b * C + c] * 2.0f * sg * (1.0f - sg);
    }
    dlog[(long)b * C + c] = dz * m;
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int lc_mvp_select(hipStream_t st, int B, int P, int W, int K, const float* query, long ldq,
                  const float* key, long ldk, const float* count, int64_t* idx, float* dist,
                  float* qnorm, float* knorm, unsigned long long* hist) {
  LC_CHECK_ARG(B > 0 && P > 0 && P <= MVP_MAXP && W > 0 && W <= MVP_MAXW && K > 0 && K <= 8 &&
               K <= P && ldq >= W && ldk >= W);
  LC_CHECK_ARG(query && key && idx && dist && qnorm && knorm);
  hipLaunchKernelGGL(mvp_select_kernel, dim3(B), dim3(256), 0, st, B, P, W, K, query, ldq, key,
                     ldk, count, idx, dist, qnorm, knorm, hist);
  LC_LAUNCH_RET();
}

int lc_mvp_simloss(hipStream_t st, int B, int P, int W, int K, int contrastiv, const float* key,
                   long ldk, const float* count, const int64_t* idx, const float* dist,
                   const float* knorm, float* kcos, float* rawgd, float* rawW, float* coef,
                   float* loss) {
  LC_CHECK_ARG(B > 0 && P > 0 && P <= MVP_MAXP && W > 0 && W <= MVP_MAXW && K > 0 && K <= 8 &&
               K <= P && ldk >= W && (long)B * K <= (1L << 20));
  LC_CHECK_ARG(idx && dist && rawgd && coef && loss);
  if (contrastiv) {
    // the reference's quotient key_wise_distance[topk] / mass[topk] does not broadcast for a
    // general batch at selection sizes above 1 (it raises there)
    LC_CHECK_ARG(K == 1 && key && count && knorm && kcos && rawW);
    hipLaunchKernelGGL(mvp_keycos_kernel, dim3(P), dim3(256), 0, st, P, W, key, ldk, knorm, kcos);
  }
  hipLaunchKernelGGL(mvp_simloss_kernel, dim3(1), dim3(256), 0, st, B, P, K, contrastiv, count,
                     idx, dist, kcos, rawgd, rawW, coef, loss);
  LC_LAUNCH_RET();
}

int lc_mvp_simloss_bwd(hipStream_t st, int B, int P, int W, int K, int contrastiv,
                       const float* query, long ldq, const float* key, long ldk,
                       const int64_t* idx, const float* dist, const float* qnorm,
                       const float* knorm, const float* kcos, const float* rawgd,
                       const float* rawW, const float* coef, const float* upstream, float* dkey,
                       long ldd) {
  LC_CHECK_ARG(B > 0 && P > 0 && P <= MVP_MAXP && W > 0 && W <= MVP_MAXW && K > 0 && K <= 8 &&
               K <= P && ldq >= W && ldk >= W && ldd >= W && (long)B * K <= (1L << 20));
  LC_CHECK_ARG(query && key && idx && dist && qnorm && knorm && rawgd && coef && dkey);
  LC_CHECK_ARG(!contrastiv || (K == 1 && kcos && rawW));
  hipLaunchKernelGGL(mvp_simloss_bwd_kernel, dim3(P), dim3(256), 0, st, B, P, W, K, contrastiv,
                     query, ldq, key, ldk, idx, dist, qnorm, knorm, kcos, rawgd, rawW, coef,
                     upstream, dkey, ldd);
  LC_LAUNCH_RET();
}

int lc_pool_gather(hipStream_t st, int B, int K, int P, long R, const float* table, long ldt,
                   const int64_t* idx, float* out, int mean) {
  LC_CHECK_ARG(B > 0 && K > 0 && K <= 8 && P > 0 && P <= MVP_MAXP && R > 0 && ldt >= R &&
               (long)B * K <= 65535);
  LC_CHECK_ARG(table && idx && out);
  const int rows = mean ? B : B * K;
  const dim3 grid((unsigned)((R + 1023) / 1024), (unsigned)rows);
  if (R % 4 == 0 && ldt % 4 == 0 && al16(table) && al16(out))
    hipLaunchKernelGGL(mvp_gather_kernel<true>, grid, dim3(256), 0, st, K, P, R, table, ldt, idx,
                       out, mean);
  else
    hipLaunchKernelGGL(mvp_gather_kernel<false>, grid, dim3(256), 0, st, K, P, R, table, ldt, idx,
                       out, mean);
  LC_LAUNCH_RET();
}

int lc_pool_gather_bwd(hipStream_t st, int B, int K, int P, long R, const int64_t* idx,
                       const float* g, long ldg, int shared_s, float alpha, float* dtable,
                       long ldd, int* ws, long ws_ints) {
  LC_CHECK_ARG(B > 0 && K > 0 && K <= 8 && P > 0 && P <= MVP_MAXP && R > 0 && ldg >= R &&
               ldd >= R && (long)B * K <= (1L << 20));
  LC_CHECK_ARG(idx && g && dtable && ws && ws_ints >= (long)P + 1 + (long)B * K);
  hipLaunchKernelGGL(mvp_sort_kernel, dim3(1), dim3(128), 0, st, B * K, P, idx, ws);
  const dim3 grid((unsigned)((R + 255) / 256), (unsigned)P);
  if (R % 4 == 0 && ldg % 4 == 0 && ldd % 4 == 0 && al16(g) && al16(dtable))
    hipLaunchKernelGGL(mvp_gather_bwd_kernel<true>, grid, dim3(64), 0, st, K, P, R, ws, g, ldg,
                       shared_s, alpha, dtable, ldd);
  else
    hipLaunchKernelGGL(mvp_gather_bwd_kernel<false>, grid, dim3(64), 0, st, K, P, R, ws, g, ldg,
                       shared_s, alpha, dtable, ldd);
  LC_LAUNCH_RET();
}

int lc_mvp_head_fwd(hipStream_t st, int B, int C, int E, const float* img_n, const float* txt_n,
                    const float* logit_scale, const float* maskrows, long ldm, const float* cmask,
                    const int64_t* labels, float* logits, float* u, float* probs, float* nll,
                    float* q1) {
  LC_CHECK_ARG(B > 0 && C > 0 && C <= 1024 && E > 0 && E <= 1024 && (!maskrows || ldm >= C));
  LC_CHECK_ARG(img_n && txt_n && logit_scale && labels && logits && u && probs && nll && q1);
  hipLaunchKernelGGL(mvp_head_fwd_kernel, dim3(B), dim3(256), 0, st, B, C, E, img_n, txt_n,
                     logit_scale, maskrows, ldm, cmask, labels, logits, u, probs, nll, q1);
  LC_LAUNCH_RET();
}

int lc_mvp_loss_mean(hipStream_t st, int B, const float* nll, const float* gsf_sum, float alpha,
                     float inv_n, float* loss, float* w, float* lbar) {
  LC_CHECK_ARG(B > 0 && nll && loss && w && lbar);
  hipLaunchKernelGGL(mvp_loss_mean_kernel, dim3(1), dim3(256), 0, st, B, nll, gsf_sum, alpha,
                     inv_n, loss, w, lbar);
  LC_LAUNCH_RET();
}

int lc_mvp_score_g(hipStream_t st, int B, int C, int E, const float* img_n, const float* probs,
                   const float* q1, const float* maskrows, long ldm, const float* logit_scale,
                   const int64_t* labels, float scale, float* G) {
  LC_CHECK_ARG(B > 0 && C > 0 && C <= 1024 && E > 0 && E <= 1024 && (!maskrows || ldm >= C));
  LC_CHECK_ARG(img_n && probs && q1 && logit_scale && labels && G);
  hipLaunchKernelGGL(mvp_score_g_kernel, dim3(C), dim3(256), 0, st, B, C, E, img_n, probs, q1,
                     maskrows, ldm, logit_scale, labels, scale, G);
  LC_LAUNCH_RET();
}

int lc_mvp_score(hipStream_t st, int B, int C, int E, const float* img_n, const float* txt_n,
                 const float* G, const float* q1, const float* maskrows, long ldm,
                 const float* logit_scale, const int64_t* labels, float margin, float gamma,
                 float* ign, float* cps, float* ign_sum) {
  LC_CHECK_ARG(B > 0 && C > 0 && C <= 1024 && E > 0 && E <= 1024 && (!maskrows || ldm >= C));
  LC_CHECK_ARG(img_n && txt_n && G && q1 && logit_scale && labels && ign && cps);
  hipLaunchKernelGGL(mvp_score_rows_kernel, dim3(B), dim3(64), 0, st, B, C, E, img_n, txt_n, G,
                     q1, maskrows, ldm, logit_scale, labels, margin, ign, cps);
  if (ign_sum)
    hipLaunchKernelGGL(mvp_ign_sum_kernel, dim3(1), dim3(256), 0, st, B, ign, gamma, ign_sum);
  LC_LAUNCH_RET();
}

int lc_mvp_afs(hipStream_t st, int B, int E, const float* img_n, const float* norms,
               const float* cps, float* out_n, float* out_norms) {
  LC_CHECK_ARG(B > 0 && E > 0 && img_n && norms && cps && out_n && out_norms);
  hipLaunchKernelGGL(mvp_afs_kernel, dim3(B), dim3(64), 0, st, B, E, img_n, norms, cps, out_n,
                     out_norms);
  LC_LAUNCH_RET();
}

int lc_mvp_head_bwd(hipStream_t st, int B, int C, int NC, const float* probs, const float* q1,
                    const float* u, const float* maskrows, long ldm, const int64_t* labels,
                    const float* w, float inv_b, float* dlog, float* dmask, long ldd) {
  LC_CHECK_ARG(B > 0 && C > 0 && C <= 1024 && NC >= C && (!maskrows || ldm >= C) &&
               (!dmask || (maskrows && ldd >= NC)));
  LC_CHECK_ARG(probs && q1 && u && labels && dlog);
  hipLaunchKernelGGL(mvp_head_bwd_kernel, dim3(B), dim3(256), 0, st, B, C, NC, probs, q1, u,
                     maskrows, ldm, labels, w, inv_b, dlog, dmask, ldd);
  LC_LAUNCH_RET();
}

}  // extern "C"
