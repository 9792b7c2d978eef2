// Stand-alone program of tests/test_routes_host.py: prints what the window-attention route functions of csrc/routes.h choose on
// a grid of (dtype, head dim, window, shift), one line per point, kernels spelled as tests/attn_cases.py spells them:
//   <dtype> <hd> <ws> <shift> | <forward> | <backward> | <window-major backward> | <recomputing backward> | <fast forward grid>
//   <persistent backward grid> <RC grid>
// with ';' between the kernels of one launch sequence and '-' for a call the entry point refuses.
#include <cstdio>
#include <string>
#include "../../small-object-detection-transformers_amd/csrc/routes.h"

static std::string ty(int dtype) { return dtype == SODT_BF16 ? "bf16" : "float"; }
static std::string args(int dtype, int hd) { return ty(dtype) + ", " + std::to_string(hd); }
static std::string args(int dtype, int hd, int nw) { return args(dtype, hd) + ", " + std::to_string(nw); }

static std::string fwd(int dtype, int hd, const AttnGeo& g) {
  const AttnRoute r = attn_fwd_route(dtype, hd, g);
  if (!r.nw) return "-";
  switch ((AttnFwdKind)r.kind) {
    case AF_FAST: return "attn_fwd_fast_kernel<" + args(dtype, hd, r.nw) + ">";
    case AF_MT2: return "attn_fwd_mt2_kernel<" + args(dtype, hd) + ">";
    case AF_MT: return "attn_fwd_mt_kernel<" + args(dtype, hd) + ">";
    case AF_GENERIC: return "attn_fwd_kernel<" + args(dtype, hd, r.nw) + ">";
  }
  return "?";
}

static std::string bwd_kind(const AttnRoute& r, int dtype, int hd, const char* wm_rc) {
  if (!r.nw) return "-";
  const std::string delta = "attn_delta_kernel<" + ty(dtype) + ">;";
  switch ((AttnBwdKind)r.kind) {
    case AB_FAST2: return "attn_bwd_fast2_kernel<" + args(dtype, hd, r.nw) + ", " + wm_rc + ">";
    case AB_SINGLE: return "attn_bwd_kernel<" + args(dtype, hd, r.nw) + ", true>";
    case AB_DKV_DQ: return delta + "attn_bwd_dkv_kernel<" + args(dtype, hd) + ">;attn_bwd_dq_kernel<" + args(dtype, hd) + ">";
    case AB_MT: return delta + "attn_bwd_mt_kernel<" + args(dtype, hd, r.nw) + ">;attn_dq_finish_kernel<" + ty(dtype) + ">";
    case AB_GENERIC: return "attn_bwd_kernel<" + args(dtype, hd, r.nw) + ", false>";
  }
  return "?";
}

int main() {
  const int heads = 12, B = 2;
  for (int dtype : {SODT_F32, SODT_BF16})
    for (int hd : {16, 32, 64})
      for (int ws : {8, 16, 32, 64})
        for (int shift : {0, ws / 2}) {
          AttnGeo g;
          if (!make_geo(g, B, 2 * ws, 2 * ws, heads * hd, heads, ws, shift)) return 1;
          const int nwin = g.B * g.nwy * g.nwx, nwb = attn_nw(dtype, hd, true);
          std::printf("%s %d %d %d | %s | %s | %s | %s | %d %d %d\n", ty(dtype).c_str(), hd, ws, shift, fwd(dtype, hd, g).c_str(),
                      bwd_kind(attn_bwd_route(dtype, hd, g), dtype, hd, "false, false").c_str(),
                      bwd_kind(attn_bwd_wm_route(dtype, hd, g), dtype, hd, "true, false").c_str(),
                      bwd_kind(attn_bwd_rc_route(dtype, g), dtype, hd, "true, true").c_str(),
                      attn_fwd_fast_grid(nwin), bwd_persistent_grid(nwin, heads / nwb, nwb), attn_rc_grid(nwin));
        }
  return 0;
}
