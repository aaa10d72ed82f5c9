// The one statement of where things lie: the order of the flat float32 weight blob (include/chiron_amd.h) and the frame counts of
// TF 'SAME' padding down the convolution stack.  The engine (engine.hip) and both training seams (cnn_grad.hip, rnn_grad.hip) read
// their offsets and their geometry from here; chiron_amd/model.py states the same order as ModelSpec.blob_layout().  Host only.
#pragma once
#include <stddef.h>

#include "../../include/chiron_amd.h"
#include "host_entry.h"
#include "kernels.h"

namespace chiron {

inline chiron_status validate_desc(const chiron_model_desc* d) {
  if (!d) return set_error(CHIRON_ERR_INVALID, "null model descriptor");
  if (d->n_blocks < 1 || d->n_blocks > CHIRON_MAX_BLOCKS) return set_error(CHIRON_ERR_INVALID, "n_blocks %d out of range", d->n_blocks);
  for (int i = 0; i < d->n_blocks; ++i) {
    const chiron_res_block& b = d->blocks[i];
    const int want_in = i == 0 ? (d->stem_k > 0 ? d->stem_channels : 1) : d->blocks[i - 1].out_channels;
    if (b.in_channels != want_in) return set_error(CHIRON_ERR_INVALID, "block %d: in_channels %d, expected %d", i, b.in_channels, want_in);
    if (b.out_channels < 4 || b.out_channels % 4) return set_error(CHIRON_ERR_INVALID, "block %d: out_channels must be a multiple of 4", i);
    if (b.k < 1 || b.k > GEMM_MAX_SEG) return set_error(CHIRON_ERR_INVALID, "block %d: conv2b width %d unsupported (1..%d)", i, b.k, GEMM_MAX_SEG);
    if (b.stride < 1) return set_error(CHIRON_ERR_INVALID, "block %d: stride %d", i, b.stride);
  }
  if (d->stem_k < 0 || d->stem_k > 64 || (d->stem_k > 0 && (d->stem_stride < 1 || d->stem_channels < 8 || d->stem_channels % 8)))
    return set_error(CHIRON_ERR_INVALID, "stem: k %d stride %d channels %d", d->stem_k, d->stem_stride, d->stem_channels);
  if (d->rnn_kind != CHIRON_RNN_STACK && d->rnn_kind != CHIRON_RNN_MULTI) return set_error(CHIRON_ERR_INVALID, "rnn_kind %d", d->rnn_kind);
  if (d->rnn_layers < 1 || d->rnn_layers > 8) return set_error(CHIRON_ERR_INVALID, "rnn_layers %d unsupported (1..8)", d->rnn_layers);
  if (d->hidden < 4 || d->hidden > 100 || d->hidden % 4) return set_error(CHIRON_ERR_INVALID, "hidden %d unsupported (multiple of 4, <= 100)", d->hidden);
  if (d->classes < 2 || d->classes > CHIRON_KMAX) return set_error(CHIRON_ERR_INVALID, "classes %d unsupported (2..%d)", d->classes, CHIRON_KMAX);
  if (d->bn_mode != CHIRON_BN_POPULATION && d->bn_mode != CHIRON_BN_BATCH) return set_error(CHIRON_ERR_INVALID, "bn_mode %d", d->bn_mode);
  return CHIRON_OK;
}

// TF 'SAME' padding: out = ceil(W/s), pad_total = max((out-1)s + k - W, 0), left = total/2
inline void same_pad(int w, int k, int s, int* out, int* left) {
  *out = (w + s - 1) / s;
  int tot = (*out - 1) * s + k - w;
  if (tot < 0) tot = 0;
  *left = tot / 2;
}

inline int lstm_in_width(const chiron_model_desc* d, int layer) {
  if (layer == 0) return d->blocks[d->n_blocks - 1].out_channels;
  return d->rnn_kind == CHIRON_RNN_STACK ? 2 * d->hidden : d->hidden;
}

// One convolution: filter [k][ci][co] at w_off, then, where bn is set, its four BN slots of co floats each (scale, offset, mean,
// variance) at bn_off.  branch1 without i_bn has no slots: its bn_off means nothing.
struct ConvSite {
  int ci, co, k, stride;
  bool bn, relu;
  size_t w_off, bn_off;
};

constexpr int MAX_SITES = 1 + 4 * CHIRON_MAX_BLOCKS;
enum { SITE_BRANCH1 = 0, SITE_CONV2A, SITE_CONV2B, SITE_CONV2C };   // site[has_stem + 4 * block + ...]

// Every offset is in floats from the start of the blob.
struct BlobMap {
  int n_sites, has_stem;
  ConvSite site[MAX_SITES];   // the stem when stem_k > 0, then branch1 / conv2a / conv2b / conv2c of every block
  size_t lstm_kernel[8][2], lstm_bias[8][2];   // [layer][direction]: kernel [in + H][4H], bias [4H]
  int lstm_in[8];
  size_t head_w, head_b, head_wc, head_bc;     // FC head: [2H], [H], [H][classes], [classes]
  size_t cnn_floats;                           // where the recurrent section starts
  size_t total;
};

inline chiron_status blob_map(const chiron_model_desc* d, BlobMap* m) {
  chiron_status st = validate_desc(d);
  if (st) return st;
  *m = BlobMap();
  size_t n = 0;
  auto conv = [&](int ci, int co, int k, int stride, bool bn, bool relu) {
    ConvSite& s = m->site[m->n_sites++];
    s = ConvSite{ci, co, k, stride, bn, relu, n, 0};
    n += (size_t)k * ci * co;
    s.bn_off = n;
    if (bn) n += 4 * (size_t)co;
  };
  m->has_stem = d->stem_k > 0;
  if (m->has_stem) conv(1, d->stem_channels, d->stem_k, d->stem_stride, true, true);
  for (int i = 0; i < d->n_blocks; ++i) {
    const chiron_res_block& b = d->blocks[i];
    conv(b.in_channels, b.out_channels, 1, b.stride, b.i_bn != 0, false);   // branch1
    conv(b.in_channels, b.out_channels, 1, 1, true, true);                  // conv2a
    conv(b.out_channels, b.out_channels, b.k, b.stride, true, true);        // conv2b
    conv(b.out_channels, b.out_channels, 1, 1, true, false);                // conv2c
  }
  m->cnn_floats = n;
  const size_t H = d->hidden, K = d->classes;
  for (int l = 0; l < d->rnn_layers; ++l) {
    m->lstm_in[l] = lstm_in_width(d, l);
    for (int dir = 0; dir < 2; ++dir) {
      m->lstm_kernel[l][dir] = n;
      n += (m->lstm_in[l] + H) * 4 * H;
      m->lstm_bias[l][dir] = n;
      n += 4 * H;
    }
  }
  m->head_w = n;
  m->head_b = m->head_w + 2 * H;
  m->head_wc = m->head_b + H;
  m->head_bc = m->head_wc + H * K;
  m->total = m->head_bc + K;
  return CHIRON_OK;
}

// The one 'SAME' walk: per site the frames it reads and writes per window and its left padding.  Both branches of a block read the
// block's input; conv2b carries the block's stride, and conv2c runs at its output length.  Returns the frames the CNN hands on.
struct SiteFrames {
  int tin, tout, pad;
};
inline int frames(const BlobMap& m, int segment_len, SiteFrames* f) {
  int t = segment_len;
  for (int i = 0; i < m.n_sites; ++i) {
    f[i].tin = t;
    same_pad(t, m.site[i].k, m.site[i].stride, &f[i].tout, &f[i].pad);
    const int in_block = i - m.has_stem;
    if (in_block < 0 || in_block % 4 == SITE_CONV2B) t = f[i].tout;
  }
  return t;
}

}  // namespace chiron
