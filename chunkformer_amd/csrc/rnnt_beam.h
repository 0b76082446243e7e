// What rnnt_beam.hip shares with rnnt_lattice.hip: the beam search's workspace regions, its GEMM operands and the
// predictor step over the rows of a call.
#pragma once
#include <hip/hip_runtime.h>

#include "beam.h"
#include "rnnt.h"

namespace cfm {

// which rows a kernel touches: utterance b's slots k < n[b] while t < ulen[b]; all of them with ulen == null
struct RbLive {
  const int32_t *ustart, *ulen, *n;
  int K, t;
};

struct RbWS {
  int32_t *err, *ustart, *ulen, *n, *node, *tok, *tptr, *par, *chg, *ti;
  double* score;
  float* tv;
  TrieRegions trie;
  size_t zero_bytes;   // [err, enc_proj): zeroed before a search
  float* enc_proj;
  float *xh[RNNT_MAXL][2], *c[RNNT_MAXL][2], *hn[RNNT_MAXL], *cn[RNNT_MAXL];
  float *gates, *pj, *z, *logits;
  size_t act_off, act_bytes;   // the activations: zeroed before a search (the initial LSTM state)
  // a stateless handle: the K_c - 1 ids before each slot's last token (-1 = before the sos), two buffers; the last
  // token as the context kernel saw it (the prune kernel overwrites tok); the mixed vector and the predictor output
  int32_t *hist[2], *ptok;
  size_t hist_off, hist_bytes;   // set to 0xff (-1) before a search
  float *sx, *sy;
};

// the GEMM operands in [N][K] layout, once per handle (0 = ok)
int rb_weights(cfm_rnnt* h);
RbWS rb_carve(const cfm_rnnt* h, void* base, int rows, int B, int K, size_t* total);
bool rb_geom_ok(const cfm_rnnt* h, int rows, int B, int K);
// gemm<float> walks K in steps of 32
bool rb_widths_ok(const cfm_rnnt* h);
int rb_gemm(const float* A, int lda, const float* W, const float* bias, int M, int N, int Kd, float* out, int ldo,
            hipStream_t st);
// embedding, LSTM layers, composed projection + pred_ffn for the live rows: state (h in xh[l][cur]'s h part, c in
// c[l][cur]) -> hn / cn (the state after this token) and pj
cfm_status rb_predictor(const cfm_rnnt* h, const RbWS& s, const RbLive& lv, int R, int cur, hipStream_t st);
// The stateless predictors for the live rows: row r's window is hist[r * hist_ld .. + Kc - 1) then last[r * last_ld]
// (ids, -1 = a zero vector) -> x (mix), y (predictor output) [R, E], pj = pred_ffn(y) [R, J]; ptok (or null) receives
// the last id of every live row
cfm_status sl_predictor(const cfm_rnnt* h, const RbLive& lv, const int32_t* hist, int hist_ld, const int32_t* last,
                        int last_ld, int R, int32_t* ptok, float* x, float* y, float* pj, hipStream_t st);
// ustart / ulen / the start beam of every utterance (a bad row range sets the error word and counts as no rows)
int rb_init(const int32_t* row_start, const int32_t* row_len, int B, int K, int rows, int max_len, int blank,
            const RbWS& s, hipStream_t st);

}  // namespace cfm
