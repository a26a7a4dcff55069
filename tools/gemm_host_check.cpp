// Host side of csrc/gemm.hip under a sanitizer, stand-alone (no GPU, no Python):
//
//   cd lifelong-clip_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     gemm.hip blaslt.hip ../../tools/gemm_host_check.cpp -o build/gemm_host_check \
//     -L/opt/rocm/lib -lhipblaslt -Wl,-rpath,/opt/rocm/lib && build/gemm_host_check > cells.txt
//
// It prints lc_gemm_split_plan over the sweep of tools/gemm_plan_sweep.py in that tool's format
// (diff the two outputs), then calls lc_gemm_nt / _ws / _rows / _fp8 once per argument check with
// an argument that check rejects. Every such call returns before any launch; the program fails if
// one returns another code than expected.
#include <stdint.h>
#include <stdio.h>

#include "lc_clip.h"

static int failures = 0, calls = 0;
static void expect(int line, int rc, int want) {
  ++calls;
  if (rc != want) {
    ++failures;
    fprintf(stderr, "line %d: returned %d, expected %d\n", line, rc, want);
  }
}
#define REJECT(call) expect(__LINE__, call, LC_EINVAL)
#define UNSUPPORTED(call) expect(__LINE__, call, LC_EUNSUPPORTED)

alignas(256) static char buf[4096];  // never read or written: every call returns at a check

int main() {
  const int Ms[] = {64,    770,   4095,  4096,  4293,  7700,  12763, 12800, 25216,
                    25600, 27776, 28160, 32768, 50395, 50432, 65792, 75676};
  const int Ns[] = {64, 192, 256, 512, 768, 2304, 3072};
  const int Ks[] = {64, 128, 768, 1024, 2048, 2304, 3072};
  const int knobs[][2] = {{0, 0}, {1, 0}, {0, 8}};  // (stream-K mode, forced tile)
  const long ws_full = LC_SPLITK_TICKET_BYTES + 256L * 256 * 256 * 4;  // ops.SPLITK_WS_BYTES
  long cells = 0, split = 0;
  for (auto& kn : knobs) {
    if (lc_gemm_set_streamk(kn[0]) || lc_gemm_set_tile(kn[1])) return 2;
    for (long ws : {0L, ws_full})
      for (int M : Ms)
        for (int N : Ns)
          for (int K : Ks) {
            int dp = -1, s = -1;
            const int rc = lc_gemm_split_plan(M, N, K, ws, &dp, &s);
            printf("%d %d %ld %d %d %d %d %d %d\n", kn[0], kn[1], ws, M, N, K, rc, dp, s);
            ++cells;
            split += rc == 0 && s > 1;
          }
  }
  lc_gemm_set_streamk(0);
  lc_gemm_set_tile(0);
  printf("# %ld cells, %ld with a split\n", cells, split);

  void *p = buf, *odd = buf + 8, *ws = buf;
  const long wsb = LC_SPLITK_TICKET_BYTES, big21 = 1L << 21, big22 = 1L << 22, big23 = 1L << 23;
  int dp, s;
  REJECT(lc_gemm_split_plan(0, 256, 64, 0, &dp, &s));
  REJECT(lc_gemm_split_plan(256, 256, 96, 0, &dp, &s));
  REJECT(lc_gemm_split_plan(256, 256, 64, 0, nullptr, &s));
  // lc_gemm_nt / lc_gemm_nt_ws: (stream, epi, M, N, K, A, lda, B, ldb, bias, alpha, out0, ldo0,
  // out1, ldo1, aux, ldaux[, ws, ws_bytes])
  REJECT(lc_gemm_nt(0, 0, 0, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 96, p, 96, p, 96, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 200, 64, p, 64, p, 64, 0, 1.f, p, 200, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 64, p, 68, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 128, p, 64, p, 128, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 64, p, big22, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 64, p, 64, p, big22, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 260, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 128, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, big21, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 0, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, big21, 0, 0));
  REJECT(lc_gemm_nt(0, -1, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 8, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0));   // internal
  REJECT(lc_gemm_nt(0, 12, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, p, 256, 0, 0));  // fp8 only
  REJECT(lc_gemm_nt(0, 15, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt(0, 3, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 256, 0, 0));   // out1
  REJECT(lc_gemm_nt(0, 5, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, p, 128, 0, 0));
  REJECT(lc_gemm_nt(0, 6, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, p, 260, 0, 0));
  REJECT(lc_gemm_nt(0, 2, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 256));   // aux
  REJECT(lc_gemm_nt(0, 4, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, p, 128));
  REJECT(lc_gemm_nt(0, 7, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, p, 260));
  REJECT(lc_gemm_nt(0, 14, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 256));
  REJECT(lc_gemm_nt_ws(0, 0, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0, odd, wsb));
  REJECT(lc_gemm_nt_ws(0, 0, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0, ws, wsb - 1));
  REJECT(lc_gemm_nt_ws(0, 9, 256, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 0, 0, 0, ws, wsb));
  // lc_gemm_nt_rows: (stream, epi, n, N, K, A, lda, B, ldb, bias, alpha, out, ldo, M_full, mul,
  // add, ws, ws_bytes)
  const float* fb = reinterpret_cast<const float*>(buf);
  REJECT(lc_gemm_nt_rows(0, 0, 0, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 1, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 96, p, 96, p, 96, 0, 1.f, p, 256, 256, 1, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 0, 1, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 0, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 1, -1, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 32, 32, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 1, 0, odd, wsb));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 1, 0, ws, wsb - 1));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, 0, 256, 256, 1, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, odd, 256, 256, 1, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 260, 256, 1, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 128, 256, 1, 0, 0, 0));
  REJECT(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, fb + 1, 1.f, p, 256, 256, 1, 0, 0, 0));
  UNSUPPORTED(lc_gemm_nt_rows(0, 3, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 1, 0, 0, 0));
  UNSUPPORTED(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 2.f, p, 256, 256, 1, 0, 0, 0));
  // the hipBLASLt shape, a forced tile, a stream-K mode
  UNSUPPORTED(lc_gemm_nt_rows(0, 0, 8, 768, 2304, p, 2304, p, 2304, 0, 1.f, p, 768, 32768, 1, 0,
                              ws, ws_full));
  lc_gemm_set_tile(8);
  UNSUPPORTED(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 1, 0, 0, 0));
  lc_gemm_set_tile(0);
  lc_gemm_set_streamk(3);
  UNSUPPORTED(lc_gemm_nt_rows(0, 0, 8, 256, 64, p, 64, p, 64, 0, 1.f, p, 256, 256, 1, 0, 0, 0));
  lc_gemm_set_streamk(0);
  // lc_gemm_nt_fp8: (stream, epi, M, N, K, A, lda, sa, sa_rows, B, ldb, sb, sb_rows, bias, alpha,
  // out0, ldo0, out1, ldo1, aux, ldaux, ws, ws_bytes, q_scale, q_rows)
#define FP8(epi, M, N, K, lda, sa, sar, ldb, sb, sbr, o0, l0, o1, l1, aux, la, w, wb, qs, qr) \
  lc_gemm_nt_fp8(0, epi, M, N, K, p, lda, sa, sar, p, ldb, sb, sbr, 0, 1.f, o0, l0, o1, l1, aux, \
                 la, w, wb, qs, qr)
  REJECT(FP8(0, 0, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 64, 64, p, 256, 64, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 128, 128, 128, p, 256, 128, p, 256, p, 128, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 136, p, 256, 128, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 256, 128, p, 256, 256, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, 0, 256, 128, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 257, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, 128, p, 300, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, odd, 256, 128, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(4, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 0, p, 256, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, 128, p, 256, 0, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, 128, p, 256, p, 260, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(3, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 256, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(12, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, p, 264, 0, 0, 0, 0, p, 256));
  REJECT(FP8(12, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, p, 256, 0, 0, 0, 0, 0, 256));
  REJECT(FP8(13, 256, 256, 128, 128, p, 256, 128, p, 256, 0, 0, p, 256, p, 256, 0, 0, p, 128));
  REJECT(FP8(2, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 0, 0, 256, 0, 0, 0, 0));
  REJECT(FP8(14, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 0, p, 128, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 0, 0, 0, odd, wsb, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, 0, 0, 0, ws, wsb - 1, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, 128, p, 256, p, big21, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, 128, p, 256, p, 256, 0, big21, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, big23, p, 256, 128, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  REJECT(FP8(0, 256, 256, 128, 128, p, 256, big23, p, 256, p, 256, 0, 0, 0, 0, 0, 0, 0, 0));
  fprintf(stderr, "%d rejected calls checked, %d wrong\n", calls, failures);
  return failures ? 1 : 0;
}
