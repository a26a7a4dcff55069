// Host side of csrc/attention.hip under a sanitizer, stand-alone (no GPU, no Python):
//
//   cd lifelong-clip_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include \
//     -fno-honor-nans -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined attention.hip ../../tools/attn_host_check.cpp \
//     -o build/attn_host_check && build/attn_host_check > codes.txt
//   (the IEEE-half build: add -DLC_F16 -include lc_f16_names.h, which renames the calls below too)
//
// One call per argument check of the nine attention entry points, each with an argument that
// check rejects, printed as "line code". Every call returns at a check, before any launch; the
// program fails if one returns another code than expected. Built on two revisions of
// attention.hip, the outputs show which rejections moved.
#include <stdint.h>
#include <stdio.h>

#include "lc_clip.h"

static int failures = 0, calls = 0;
static void expect(int line, int rc, int want) {
  ++calls;
  printf("%d %d\n", line, rc);
  if (rc != want) {
    ++failures;
    fprintf(stderr, "line %d: returned %d, expected %d\n", line, rc, want);
  }
}
#define REJECT(call) expect(__LINE__, call, LC_EINVAL)
#define UNSUPPORTED(call) expect(__LINE__, call, LC_EUNSUPPORTED)
#define ACCEPT(call) expect(__LINE__, call, LC_OK)

alignas(256) static char buf[4096];  // never read or written: every call returns at a check

int main() {
  void *p = buf, *odd = buf + 8;
  float* f = reinterpret_cast<float*>(buf);
  // 2 sequences of 64 tokens, 2 heads: D = 128, qkv / dqkv rows of 384, O rows of 128
  const long big22 = 1L << 22, big23 = 1L << 23;  // the stride bound, in elements / in bytes
  const long big21 = 1L << 21;                    // the long family's (512 padded rows)

  // lc_attn_fwd(stream, n_seq, L, H, qkv, ldq, O, ldo, lse, causal)
  REJECT(lc_attn_fwd(0, 0, 64, 2, p, 384, p, 128, f, 0));
  REJECT(lc_attn_fwd(0, 2, 0, 2, p, 384, p, 128, f, 0));
  REJECT(lc_attn_fwd(0, 2, 257, 2, p, 384, p, 128, f, 0));
  REJECT(lc_attn_fwd(0, 2, 64, 0, p, 384, p, 128, f, 0));
  REJECT(lc_attn_fwd(0, 2, 64, 2, p, 376, p, 128, f, 0));
  REJECT(lc_attn_fwd(0, 2, 64, 2, p, 388, p, 128, f, 0));
  REJECT(lc_attn_fwd(0, 2, 64, 2, p, 384, p, 120, f, 0));
  REJECT(lc_attn_fwd(0, 2, 64, 2, p, 384, p, 132, f, 0));
  REJECT(lc_attn_fwd(0, 2, 64, 2, p, 384, odd, 128, f, 0));
  REJECT(lc_attn_fwd(0, 2, 64, 2, p, big22, p, 128, f, 0));  // the offset bound, new here
  REJECT(lc_attn_fwd(0, 2, 64, 2, p, 384, p, big22, f, 0));  // the offset bound, new here

  // lc_attn_bwd(stream, n_seq, L, H, qkv, ldq, O, dO, ldo, lse, dqkv, lddq, causal)
  REJECT(lc_attn_bwd(0, 0, 64, 2, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 0, 2, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 257, 2, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 0, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 376, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 388, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 384, p, p, 120, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 384, p, p, 132, f, p, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 384, p, p, 128, f, p, 376, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 384, p, p, 128, f, p, 388, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 384, p, p, 128, f, odd, 384, 0));
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, big22, p, p, 128, f, p, 384, 0));  // the bound, new here
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 384, p, p, big22, f, p, 384, 0));  // the bound, new here
  REJECT(lc_attn_bwd(0, 2, 64, 2, p, 384, p, p, 128, f, p, big22, 0));  // the bound, new here

  // lc_attn_bwd_fp8(stream, n_seq, L, H, qkv, ldq, O, dO, ldo, lse, dqkv, lddq BYTES, q_scale,
  // q_rows, causal)
  REJECT(lc_attn_bwd_fp8(0, 0, 64, 2, p, 384, p, p, 128, f, p, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 0, 2, p, 384, p, p, 128, f, p, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 225, 2, p, 384, p, p, 128, f, p, 384, p, 512, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 0, p, 384, p, p, 128, f, p, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 376, p, p, 128, f, p, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 388, p, p, 128, f, p, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 120, f, p, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 132, f, p, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 128, f, p, 368, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 128, f, p, 392, p, 256, 0));  // % 16
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 128, f, odd, 384, p, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 128, f, p, 384, 0, 256, 0));
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 128, f, p, 384, p, 128, 0));  // % 256
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 128, f, p, 384, p, 0, 0));    // < rows
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, big22, p, p, 128, f, p, 384, p, 256, 0));  // new here
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, big22, f, p, 384, p, 256, 0));  // new here
  REJECT(lc_attn_bwd_fp8(0, 2, 64, 2, p, 384, p, p, 128, f, p, big23, p, 256, 0));  // new here

  // lc_attn_row_fwd(stream, n_seq, L, H, qkv, ldq, row, O_row, ldo, lse_row, causal)
  REJECT(lc_attn_row_fwd(0, 0, 64, 2, p, 384, 0, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 0, 2, p, 384, 0, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 257, 2, p, 384, 0, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 0, p, 384, 0, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 2, p, 384, -1, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 2, p, 384, 64, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 2, p, 376, 0, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 2, p, 388, 0, p, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 2, p, 384, 0, p, 120, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 2, p, 384, 0, p, 132, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 64, 2, p, 384, 0, odd, 128, f, 0));
  REJECT(lc_attn_row_fwd(0, 2, 256, 2, p, big22, 0, p, 128, f, 0));  // the bound, at 256 rows

  // lc_attn_row_bwd / lc_attn_bwd_live_row(stream, n_seq, L, H, qkv, ldq, row, O_row, dO_row, ldo,
  // lse_row, dqkv, lddq, causal): the same checks (L <= 32 * ROW_IT = 256 / L <= 256)
#define ROW_BWD_CHECKS(fn)                                                     \
  REJECT(fn(0, 0, 64, 2, p, 384, 0, p, p, 128, f, p, 384, 0));                 \
  REJECT(fn(0, 2, 0, 2, p, 384, 0, p, p, 128, f, p, 384, 0));                  \
  REJECT(fn(0, 2, 257, 2, p, 384, 0, p, p, 128, f, p, 384, 0));                \
  REJECT(fn(0, 2, 64, 0, p, 384, 0, p, p, 128, f, p, 384, 0));                 \
  REJECT(fn(0, 2, 64, 2, p, 384, -1, p, p, 128, f, p, 384, 0));                \
  REJECT(fn(0, 2, 64, 2, p, 384, 64, p, p, 128, f, p, 384, 0));                \
  REJECT(fn(0, 2, 64, 2, p, 376, 0, p, p, 128, f, p, 384, 0));                 \
  REJECT(fn(0, 2, 64, 2, p, 388, 0, p, p, 128, f, p, 384, 0));                 \
  REJECT(fn(0, 2, 64, 2, p, 384, 0, p, p, 120, f, p, 384, 0));                 \
  REJECT(fn(0, 2, 64, 2, p, 384, 0, p, p, 132, f, p, 384, 0));                 \
  REJECT(fn(0, 2, 64, 2, p, 384, 0, p, p, 128, f, p, 376, 0));                 \
  REJECT(fn(0, 2, 64, 2, p, 384, 0, p, p, 128, f, p, 388, 0));                 \
  REJECT(fn(0, 2, 64, 2, p, 384, 0, odd, p, 128, f, p, 384, 0));               \
  REJECT(fn(0, 2, 64, 2, p, 384, 0, p, odd, 128, f, p, 384, 0));               \
  REJECT(fn(0, 2, 64, 2, p, 384, 0, p, p, 128, f, odd, 384, 0));               \
  REJECT(fn(0, 2, 256, 2, p, big22, 0, p, p, 128, f, p, 384, 0)); /* bound */   \
  REJECT(fn(0, 2, 256, 2, p, 384, 0, p, p, 128, f, p, big22, 0)); /* bound */
  ROW_BWD_CHECKS(lc_attn_row_bwd)
  ROW_BWD_CHECKS(lc_attn_bwd_live_row)

  // lc_attn_long_fwd / lc_attn_long_bwd: lc_attn_fwd / lc_attn_bwd's arguments, 257 <= L <= 512
  // (2 sequences of 257 tokens), every stride below 2^21 elements
  REJECT(lc_attn_long_fwd(0, 0, 257, 2, p, 384, p, 128, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 256, 2, p, 384, p, 128, f, 0));  // lc_attn_fwd's length
  REJECT(lc_attn_long_fwd(0, 2, 513, 2, p, 384, p, 128, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 257, 0, p, 384, p, 128, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 257, 2, p, 376, p, 128, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 257, 2, p, 388, p, 128, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 257, 2, p, 384, p, 120, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 257, 2, p, 384, p, 132, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 257, 2, p, 384, odd, 128, f, 0));
  REJECT(lc_attn_long_fwd(0, 2, 512, 2, p, big21, p, 128, f, 0));  // the bound, at 512 rows
  REJECT(lc_attn_long_fwd(0, 2, 257, 2, p, 384, p, big21, f, 0));
  REJECT(lc_attn_long_bwd(0, 0, 257, 2, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 256, 2, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 513, 2, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 0, p, 384, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 376, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 388, p, p, 128, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 384, p, p, 120, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 384, p, p, 132, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 384, p, p, 128, f, p, 376, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 384, p, p, 128, f, p, 388, 0));
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 384, p, p, 128, f, odd, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 512, 2, p, big21, p, p, 128, f, p, 384, 0));  // the bound
  REJECT(lc_attn_long_bwd(0, 2, 257, 2, p, 384, p, p, big21, f, p, 384, 0));
  REJECT(lc_attn_long_bwd(0, 2, 512, 2, p, 384, p, p, 128, f, p, big21, 0));
  // (lc_attn_bwd_set_form does not reach the long family: the same rejection under every form)
  for (int form = 1; form <= 3; ++form) {
    ACCEPT(lc_attn_bwd_set_form(form));
    REJECT(lc_attn_long_bwd(0, 2, 256, 2, p, 384, p, p, 128, f, p, 384, 0));
  }
  ACCEPT(lc_attn_bwd_set_form(0));

  // lc_attn_bwd_set_form: 0..3; lc_attn_bwd_live_row refuses under forms 2 and 3 (valid
  // arguments: it returns before any launch), after its argument checks
  REJECT(lc_attn_bwd_set_form(-1));
  REJECT(lc_attn_bwd_set_form(4));
  for (int form = 0; form <= 3; ++form) ACCEPT(lc_attn_bwd_set_form(form));
  for (int form = 2; form <= 3; ++form) {
    ACCEPT(lc_attn_bwd_set_form(form));
    UNSUPPORTED(lc_attn_bwd_live_row(0, 2, 64, 2, p, 384, 0, p, p, 128, f, p, 384, 0));
    UNSUPPORTED(lc_attn_bwd_live_row(0, 2, 256, 2, p, 384, 0, p, p, 128, f, p, 384, 0));
    REJECT(lc_attn_bwd_live_row(0, 2, 64, 2, p, 384, 64, p, p, 128, f, p, 384, 0));
  }
  ACCEPT(lc_attn_bwd_set_form(0));
  fprintf(stderr, "%d calls checked, %d wrong\n", calls, failures);
  return failures ? 1 : 0;
}
