/*
 * chiron_amd.h -- C ABI of libchiron_amd.so, the MI355X (gfx950) basecalling
 * inference engine that replaces the TensorFlow session behind the reference's
 * `chiron call` hot path.
 *
 * The reference has no FFI layer; its seam is the pair of sess.run calls in
 * chiron/chiron_eval.py (feed: :335-342, drain: :403-409), formalised by the
 * SavedModel PREDICT signature in chiron/export_test.py:103-112
 *   (x, seq_len) -> (indices, values, dense_shape, logits, prob_logits, log_prob).
 * Every entry point below cites the reference interface it replaces.
 *
 * Conventions: plain pointers and sizes only; every function returns a
 * chiron_status (0 = OK) and never throws; chiron_last_error() returns a
 * thread-local description of the last failure.  Host buffers belong to the
 * caller; device buffers, streams and weights belong to the engine; result
 * pointers stay valid until the next submit on the same slot.
 */
#ifndef CHIRON_AMD_H
#define CHIRON_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHIRON_ABI_VERSION 7
#define CHIRON_MAX_BLOCKS 8
#define CHIRON_CLASSES 5 /* A,C,G,T,blank (rnn.py:25 class_n=5) */

typedef enum {
  CHIRON_OK = 0,
  CHIRON_ERR_INVALID = 1,   /* bad argument / unsupported topology          */
  CHIRON_ERR_DEVICE = 2,    /* HIP runtime failure (no GPU, OOM, launch)     */
  CHIRON_ERR_STATE = 3,     /* collect without submit, submit on a slot whose batch was not collected, slot out of range */
  CHIRON_ERR_OVERFLOW = 4   /* batch > max_batch, beam > limit, a tensor beyond the kernels' 32-bit addressing */
} chiron_status;

/* One residual block, chiron/cnn.py:234-262 residual_layer():
 *   branch1 = conv 1x1 (stride) [+BN iff i_bn];  branch2 = 1x1+BN+ReLU ->
 *   1xk (stride)+BN+ReLU -> 1x1+BN;  out = ReLU(branch1 + branch2).          */
typedef struct {
  int32_t in_channels;  /* 1 for the first block (raw signal)                 */
  int32_t out_channels; /* 256                                                */
  int32_t k;            /* width of conv2b: 3 (DNA), 13 (shipped RNA block 1) */
  int32_t stride;       /* stride of conv2b and branch1/conv1                 */
  int32_t i_bn;         /* BN on branch1 (only res_layer1, cnn.py:382-384)    */
} chiron_res_block;

typedef enum {
  CHIRON_RNN_STACK = 0, /* rnn.py:20-97  stack_bidirectional_dynamic_rnn (DNA) */
  CHIRON_RNN_MULTI = 1  /* rnn.py:99-174 bidirectional_dynamic_rnn(MultiRNNCell) (RNA) */
} chiron_rnn_kind;

typedef enum {
  CHIRON_BN_POPULATION = 0, /* cnn.py:125-163 batchnorm() inference branch (shipped checkpoints) */
  CHIRON_BN_BATCH = 1       /* cnn.py:166-188 simple_global_bn (HEAD code)                        */
} chiron_bn_mode;

/* Topology descriptor: what chiron_model.read_config (chiron_model.py:37-48)
 * plus the checkpoint's variable shapes determine.
 *
 * What is accepted (every refusal is CHIRON_ERR_INVALID with its reason, from chiron_engine_plan or chiron_engine_create before any
 * kernel runs; tests/topology_cases.py runs or pins every line):
 *   blocks       1 .. CHIRON_MAX_BLOCKS; in_channels = the previous block's out_channels (the stem's, or 1, for the first);
 *                out_channels any multiple of 4; k 1 .. 16; stride >= 1; i_bn on any block
 *   stem         k 0 (none) .. 64, stride >= 1, channels any multiple of 8
 *   recurrence   either kind, 1 .. 8 layers, hidden 100 (the descriptor of the training seams takes no other either)
 *   classes      2 .. 5 for greedy decoding; max_beam > 0 needs 5
 *   bn_mode      CHIRON_BN_BATCH: CHIRON_F32 only, and at most 1024 output channels in any convolution
 *   dtype        CHIRON_F32: all of the above.  CHIRON_F16, CHIRON_F16_W2, CHIRON_F32_SPLIT: blocks of 1 -> 256 and 256 -> 256 channels
 *                only (a stem, if any, of 256); CHIRON_F16_W2 with a conv2b wider than 8 only on the first block of a model without
 *                a stem, where it runs as a table                                                                            */
typedef struct {
  int32_t n_blocks;
  chiron_res_block blocks[CHIRON_MAX_BLOCKS];
  int32_t rnn_kind;   /* chiron_rnn_kind                                      */
  int32_t rnn_layers; /* 3                                                    */
  int32_t hidden;     /* 100                                                  */
  int32_t classes;    /* 5                                                    */
  int32_t bn_mode;    /* chiron_bn_mode                                       */
  /* Optional stem in front of the residual blocks: HEAD's RNA_model2 / RNA_model3 (cnn.py:454-476) start with
   *   conv_layer(net, [1, k, 1, C], 'SAME', strides = s) + BN + ReLU  (k, s = 9, 5 / 14, 7; C = 256)
   * under the variable scope conv_layer/conv1.  stem_k = 0: no stem, blocks[0].in_channels must be 1 (DNA_model1 and
   * the shipped RNA graph).  With a stem, blocks[0].in_channels = stem_channels.                                 */
  int32_t stem_k, stem_stride, stem_channels;
} chiron_model_desc;

/* Weight blob layout (float32, little endian), in this order:
 *  if stem_k: conv_layer/conv1/weights [k][1][C], conv1_bn scale, offset, pop_mean, pop_var   4 x [C]
 *  for each block b:
 *     branch1/conv1/weights            [1][in][out]        (TF HWIO, H squeezed)
 *     if i_bn: conv1_bn scale, offset, pop_mean, pop_var   4 x [out]
 *     branch2/conv2a/weights           [1][in][out]
 *     conv2a_bn scale, offset, pop_mean, pop_var           4 x [out]
 *     branch2/conv2b/weights           [k][out][out]
 *     conv2b_bn ...                                        4 x [out]
 *     branch2/conv2c/weights           [1][out][out]
 *     conv2c_bn ...                                        4 x [out]
 *  for each rnn layer l, for dir in (fw, bw):
 *     lstm_cell/kernel                 [(in_l + H)][4H]    columns i|j|f|o
 *     lstm_cell/bias                   [4H]
 *       in_l: layer 0 -> out_channels of the last block;
 *             STACK l>0 -> 2H ; MULTI l>0 -> H
 *  rnn_fnn_layer/weights [2][H], bias [H], weights_class [H][K], bias_class [K]
 * (in CHIRON_BN_BATCH mode the pop_mean/pop_var slots are present but unused.) */
chiron_status chiron_weights_size(const chiron_model_desc* desc, size_t* n_floats);

/* CHIRON_F32: exact-fp32 path (fp32 MFMA), the parity path: logits within 1e-4 of the reference arithmetic.
 * CHIRON_F16: activations, weights and the recurrent h as IEEE halves on the f16 MFMA instructions; accumulation,
 *             the LSTM pre-activations z, gates, cell state, logits and both CTC decoders stay fp32 (BASELINE
 *             configs[4]); the LAST recurrent layer's output -- what the FC head reads -- leaves the recurrence as fp32 (round 6).
 *             Logits stay within 0.08 of the fp32 engine on the synthetic weights (tests/test_gpu_parity.py); identical-window rates
 *             against the fp32 engine per regime: profiles/r06_f16_frontier.json.
 * CHIRON_F32_SPLIT: fp32 VALUES, carried between kernels as hi + lo half pairs (x = hi + lo to 2^-22: 22-bit operands) and multiplied
 *             on the f16 matrix cores as hi*hi + hi*lo + lo*hi with fp32 accumulation (the f16 MFMA rate is 16x the fp32 one on
 *             gfx950); GEMM weight rows are stored scaled by a power of two so that their lo halves are normal halves; gates, z, logits
 *             and CTC are the fp32 code.  Opt-in.  What it meets (tests): the 1e-4 logits bound against the oracle on the seeded
 *             synthetic weights, as CHIRON_F32 does; on trained-checkpoint-like weights, where no float32 pipeline meets 1e-4, it is
 *             judged against the same ensemble of float32 realisations as CHIRON_F32 with wider bars (bulk rms <= 1.5 x the ensemble's
 *             p90, typical window <= 1.75 x its median; measured 0.75 .. 1.4 and 1.0 .. 1.6 -- CHIRON_F32: 0.63 .. 1.15 and 1.13 .. 1.23);
 *             greedy strings at basecalling density as CHIRON_F32.  It is not fp32 MFMA arithmetic, so the headline benchmark stays
 *             on CHIRON_F32.  Population BN only.
 * CHIRON_F16_W2: CHIRON_F16's activations (halves) against EXACT weights: every weight is carried as a hi + lo half pair
 *             (W = hi + lo to 2^-22) and every product is x*lo + x*hi on the f16 matrix cores, fp32 accumulation; the LSTM
 *             pre-activations z stay fp32 in memory.  What half precision costs this network is mostly the WEIGHTS'
 *             rounding (tools/f16_study.py: 10 x the activations'), and no calibration data is needed to avoid it:
 *             the mode for trained checkpoints when CHIRON_F16's accuracy is not enough.  Population BN only.     */
typedef enum { CHIRON_F32 = 0, CHIRON_F16 = 1, CHIRON_F32_SPLIT = 2, CHIRON_F16_W2 = 3 } chiron_dtype;

typedef struct {
  int32_t device_id;    /* HIP device ordinal                                 */
  int32_t max_batch;    /* FLAGS.batch_size (chiron_eval.py:248)              */
  int32_t segment_len;  /* FLAGS.segment_len                                  */
  int32_t n_slots;      /* in-flight batches (>=1); each has its own stream   */
  int32_t dtype;        /* chiron_dtype; CHIRON_F32 is the parity path        */
  int32_t max_beam;     /* largest beam_width that will be requested (0=greedy only) */
} chiron_engine_opts;

typedef struct chiron_engine chiron_engine;

/* Replaces build_eval_graph + Saver.restore (chiron_eval.py:244-276).        */
chiron_status chiron_engine_create(const chiron_model_desc* desc, const float* weights, size_t n_floats,
                                   const chiron_engine_opts* opts, chiron_engine** out);
void chiron_engine_destroy(chiron_engine* e);

/* Sizes of the engine chiron_engine_create would build for (desc, opts), WITHOUT touching a GPU: frame count and ratio,
 * the largest tensor the kernels address with 32-bit byte offsets against their limit, device bytes per slot and in
 * total.  Returns CHIRON_ERR_OVERFLOW (with the largest max_batch that fits in the message) when a tensor would pass
 * the limit -- e.g. fp32, segment_len 400, 256 channels: max_batch > 10485 -- and chiron_engine_create refuses the
 * same configurations with the same status instead of reading zeros past the descriptor's range.                  */
typedef struct {
  int32_t T;
  double ratio;
  uint64_t largest_tensor_bytes;
  uint64_t tensor_limit_bytes;
  uint64_t slot_bytes;
  uint64_t total_bytes;
} chiron_engine_sizes;
chiron_status chiron_engine_plan(const chiron_model_desc* desc, const chiron_engine_opts* opts, chiron_engine_sizes* out);

/* T = number of logits frames per segment and ratio = segment_len / T
 * (chiron_model.py:151-152).                                                 */
chiron_status chiron_engine_dims(const chiron_engine* e, int32_t* out_T, double* out_ratio);

/* Threading: one producer thread (submit / decode) and one consumer thread (collect) per engine may run concurrently;
 * a slot alternates strictly submit -> collect (its state is an atomic, a second submit before the collect returns
 * CHIRON_ERR_STATE and changes nothing).  Engines on different devices are independent.  A submit that fails after
 * it has started to enqueue work drains the slot's stream before returning; the slot stays free.
 *
 * flags for submit */
#define CHIRON_X_ON_DEVICE 1u   /* x / seq_len are device pointers on opts.device_id.  The slot streams are non-blocking
                                   streams and are NOT ordered against the caller's: the buffers must be complete before
                                   the call (synchronise the producing stream) and untouched until the collect          */
#define CHIRON_WANT_PROB 2u     /* compute prob_logits = path_prob (chiron_eval.py:116-136, -e fastq) */
#define CHIRON_WANT_LOGITS 4u   /* copy logits [B,T,K] back on collect                */
#define CHIRON_NO_DECODE_COPY 8u /* leave decoded sparse tensor on the device (bench)  */
#define CHIRON_COMPACT_DECODE 16u /* the host wants the decode in the per-row form of the regroup step (chiron_eval.py:403-446): collect
                                    fills flat_labels / row_counts and does NOT copy indices / values (NULL; nnz and dense_shape are
                                    still reported).  One fixed-size copy enqueued with the batch instead of a second round trip
                                    for nnz * 24 bytes of int64 pairs that the host would only scan for row boundaries.           */

/* Replaces sess.run(logits_enqueue, feed_dict) (chiron_eval.py:335-342) plus the
 * decode sub-graph (chiron_eval.py:465-492).  x: float32 [batch, segment_len]
 * row-major; seq_len: int32 [batch], ALREADY divided by ratio and rounded
 * half-even by the caller (chiron_eval.py:337).  beam_width 0 = greedy
 * (merge_repeated=True), >0 = CTC beam search (merge_repeated=False, top_paths=1).
 * Asynchronous: work is enqueued on the slot's stream.                         */
chiron_status chiron_engine_submit(chiron_engine* e, int32_t slot, const float* x, const int32_t* seq_len,
                                   int32_t batch, int32_t beam_width, uint32_t flags);

/* Decode-only: the decode sub-graph of the reference (decoding_queue, chiron_eval.py:465-492: path_prob +
 * ctc_greedy_decoder / ctc_beam_search_decoder) on caller-supplied logits float32 [batch, T, K] (T from
 * chiron_engine_dims).  Same flags, slot and collect protocol as chiron_engine_submit.                  */
chiron_status chiron_engine_decode(chiron_engine* e, int32_t slot, const float* logits, const int32_t* seq_len,
                                   int32_t batch, int32_t beam_width, uint32_t flags);

/* The reference's decoded tuple (chiron_eval.py:403-409): SparseTensor
 * (indices, values, dense_shape) + log_prob + prob_logits (+ logits).          */
typedef struct {
  int64_t nnz;
  const int64_t* indices;   /* [nnz,2] (row, position), row-major sorted        */
  const int64_t* values;    /* [nnz] in 0..3                                    */
  int64_t dense_shape[2];   /* [batch, max decoded length]                      */
  const float* log_prob;    /* [batch,1] greedy: -sum max logit; beam: log p    */
  const float* prob_logits; /* [batch,1] path_prob, or zeros without WANT_PROB  */
  const float* logits;      /* [batch,T,K] or NULL                              */
  int32_t batch;
  int32_t T;
  /* CHIRON_COMPACT_DECODE only (else NULL): the rows' decoded labels 0..3 back to back in row order [nnz], and the number of
   * labels of every row [batch] -- the same decode as (indices, values): row b owns the next row_counts[b] entries.       */
  const uint8_t* flat_labels;
  const int32_t* row_counts;
} chiron_decoded;

/* chiron_engine_submit with the batch given as `n_pieces` host arrays of whole rows (piece i: piece_rows[i] rows of segment_len
 * floats, rows summing to `batch`): the cross-read packing of chiron_eval.py:321-334 -- the tail of one read, whole reads, the
 * head of the next -- copied straight into the slot's pinned staging buffer, so the caller never assembles the [batch,
 * segment_len] array (1.76 MB per 1100-window batch on the host's main thread otherwise).  piece_row_stride[i] (floats; NULL =
 * segment_len everywhere) is the distance between consecutive rows of piece i: with stride = jump the rows ARE the windows
 * signal[r*jump : r*jump + segment_len] of one zero-padded signal buffer (chiron_input.py:276-286) and the host never
 * materialises the windowed read either.  Host pointers only.                                                            */
chiron_status chiron_engine_submit_pieces(chiron_engine* e, int32_t slot, const float* const* pieces, const int32_t* piece_rows,
                                          const int64_t* piece_row_stride, int32_t n_pieces, const int32_t* seq_len, int32_t batch,
                                          int32_t beam_width, uint32_t flags);

/* Replaces sess.run(decode dequeue) (chiron_eval.py:403-409).  Blocks until the
 * slot's work is complete, then fills *out with host pointers owned by the slot. */
chiron_status chiron_engine_collect(chiron_engine* e, int32_t slot, chiron_decoded* out);

/* Blocks until every slot's stream is idle. */
chiron_status chiron_engine_sync(chiron_engine* e);

/* Device pointers of a slot's most recent results (valid after collect/sync):
 * logits [B,T,K] f32, and the decoded sparse tensor left on device.            */
chiron_status chiron_engine_device_results(chiron_engine* e, int32_t slot, const float** logits,
                                           const int64_t** indices, const int64_t** values,
                                           const int64_t** nnz_and_shape /* [3]: nnz,batch,maxlen */);

/* getcnnfeature (cnn.py:334-371): the CNN feature tensor [batch, T, C] (float32; an f16 engine's halves are widened)
 * of the batch most recently run on `slot`, which must be idle (collected).  Copied into out [cap_floats];
 * *out_batch / *out_channels receive batch and C.  CHIRON_ERR_OVERFLOW when cap_floats is too small (the sizes are
 * still reported), CHIRON_ERR_STATE before the first batch or with a batch in flight.  Stage-level parity checks use
 * it (tests); dtype CHIRON_F32_SPLIT returns hi + lo of its half pairs.                                          */
chiron_status chiron_engine_features(chiron_engine* e, int32_t slot, float* out, size_t cap_floats, int32_t* out_batch,
                                     int32_t* out_channels);

/* The recurrent stack's output, rnn.py:63-65 (DNA: stack_bidirectional_dynamic_rnn) / rnn.py:140-145 (RNA: MultiRNNCell inside
 * bidirectional_dynamic_rnn) -- `lasth`, the tensor the FC head of rnn.py:72-96 reads: [batch, T, 2 * hidden] float32 ([..., :H]
 * forward, [..., H:] backward; frames at or past a row's seq_len are 0), of the batch most recently run on `slot` (idle).  Same
 * protocol and status codes as chiron_engine_features.  With a model descriptor of 1 or 2 rnn_layers it is the output of that
 * layer: the per-stage error budget of the parity tests (tools/parity_budget.py) is built on it.                        */
chiron_status chiron_engine_rnn_output(chiron_engine* e, int32_t slot, float* out, size_t cap_floats, int32_t* out_batch,
                                       int32_t* out_width);

/* f16 engines only (CHIRON_F16; a no-op returning CHIRON_OK for the other dtypes): bias correction for the weights' rounding to
 * halves.  The reference has no counterpart (it computes in fp32); this is what lets the f16 engine be used on a trained checkpoint
 * whose BN sites cancel large convolution means (tools/f16_study.py: there most of what half-precision WEIGHTS cost is a constant
 * per output channel, sum_k E[x_k] (f16(W) - W)[n][k]).  The call runs `batch` calibration windows (same x / seq_len convention as
 * chiron_engine_submit, host pointers) through the network `iterations` times (2 is enough; upstream corrections move downstream
 * means slightly), measures the mean of every input channel of every f16 weight matrix -- convolutions, LSTM input and recurrent
 * kernels -- and moves that constant out of the folded BN shift / LSTM bias.  No run-time cost afterwards.  Every slot must be idle.
 * iterations = 0 restores the uncorrected shifts (x, seq_len and batch are then ignored and may be NULL / 0).  An input that cannot
 * be measured (more than 256 channels; more than 256 measured inputs) is CHIRON_ERR_OVERFLOW with nothing applied.  The correction depends on the calibration windows through per-channel MEANS
 * only; `chiron call --dtype fp16` calibrates on a fixed synthetic squiggle, so every rank of a sharded run holds the same engine. */
chiron_status chiron_engine_calibrate(chiron_engine* e, const float* x, const int32_t* seq_len, int32_t batch, int32_t iterations);

/* Per-kernel timing with HIP events on the engine's own streams (bench.py
 * roofline).  Enable, run, sync, then read.                                    */
typedef struct {
  char name[48];
  double total_ms;     /* sum of hipEventElapsedTime over launches              */
  int64_t launches;
  double flops;        /* algorithmic FLOPs summed over those launches          */
  double bytes;        /* algorithmic HBM bytes summed over those launches      */
} chiron_kernel_stat;
chiron_status chiron_engine_profile(chiron_engine* e, int32_t enable);
chiron_status chiron_engine_profile_read(chiron_engine* e, chiron_kernel_stat* stats, int32_t max_stats,
                                         int32_t* n_stats);

/* Overlap-consensus vote, chiron/utils/easy_assembler.py:
 *   glue_kernal :276-294, stick_kernal :296-300, simple_assembly_kernal :212-250 (difflib.SequenceMatcher matching
 *   blocks + offset prior; `error_rate`, `jump_step_ratio` as in simple_assembly(bpreads, jump_step_ratio, error_rate,
 *   kernal) :302), simple_assembly(_qs) :302-335 / :393-432, add_count(_qs) :381-387 / :435-442, and the argmax of
 *   chiron_eval.py:457.
 * bases: concatenated segments as 0..3; seg_off [n_seg+1] prefix offsets; seg_qs [n_seg] per-segment quality (may be
 * NULL); kernal: one of CHIRON_KERNAL_*; error_rate / jump_step_ratio are read by the simple kernel only.
 * Outputs (caller-allocated, capacity cap columns): counts [4][cap] float64, qs_sum [4][cap] float64 (if seg_qs),
 * *out_len = consensus length.  Returns CHIRON_ERR_OVERFLOW if cap is too small (then *out_len = needed).
 * Pure host code: callable without a GPU and from several threads at once.                                      */
#define CHIRON_KERNAL_GLUE 1
#define CHIRON_KERNAL_STICK 2
#define CHIRON_KERNAL_SIMPLE 3
chiron_status chiron_assemble(const uint8_t* bases, const int64_t* seg_off, int64_t n_seg, const double* seg_qs,
                              int32_t kernal, double error_rate, double jump_step_ratio, double* counts, double* qs_sum,
                              int64_t cap, int64_t* out_len);

/* One read from its decoded windows to its files (chiron_eval.py:446-462 + write_output :176-228) in one call that never
 * enters the interpreter: index2base of every window, the vote above, np.argmax (:457), qs (:152-174; seg_qs = NULL or
 * fastq = 0: no quality, FASTA), then result_path = "@name\nSEQ\n+\nQUAL\n" (FASTQ) or ">name\nSEQ" (FASTA, no final
 * newline; rna != 0 writes U for T in the consensus, :204-205) and -- unless segments_path is NULL (--concise) --
 * ">name<k>\nSEGMENT\n" per window.  *consensus_len receives len(SEQ) (the caller writes meta/<name>.meta from it) and
 * consensus_out [consensus_cap], when given, SEQ itself (no terminator; the decoded base count is always enough room).
 * The folders must exist.  Equal, byte for byte, to the Python writers of chiron_amd/eval.py (tests).               */
chiron_status chiron_finish_read(const uint8_t* bases, const int64_t* seg_off, int64_t n_seg, const double* seg_qs,
                                 int32_t kernal, double error_rate, double jump_step_ratio, const char* name,
                                 const char* result_path, const char* segments_path, int32_t fastq, int32_t rna,
                                 char* consensus_out, int64_t consensus_cap, int64_t* consensus_len);

/* One displacement of the vote above: where `cur` starts relative to the start of `prev` (the return value of
 * glue_kernal / stick_kernal / simple_assembly_kernal; for the simple kernel *log_px receives its second return
 * value, the score of the chosen offset; 0 otherwise; log_px may be NULL).                                       */
chiron_status chiron_overlap_displacement(const uint8_t* cur, int64_t n, const uint8_t* prev, int64_t prev_n,
                                          int32_t kernal, double error_rate, double jump_step_ratio, int64_t* disp,
                                          double* log_px);

/* The same consensus on the device, for one read (very long reads): glue / stick displacements of every
 * consecutive segment pair, running start columns, the vote, and per consensus column the winning base
 * (np.argmax(consensus, axis=0), chiron_eval.py:457: first maximum) and, when seg_qs is given, the three numbers
 * qs() (chiron_eval.py:152-174) reads of a column: n1 and n2, the two largest vote counts, and q_top, the summed segment
 * quality behind the winning base (the last of equal maxima) -- i.e. chiron_assemble + argmax + the inputs of qs without
 * the [4][len] matrices ever leaving the GPU.  All of it is integer work or ordered double sums: identical to the host
 * vote.  The Phred character q = int(10 log10((n1+1)/(n2+1)) + q_top/n1/ln 10) is left to the caller's own formula
 * (chiron_amd.eval.qs_from_votes), because truncation turns a last-bit difference between two log10 implementations
 * into a different character.  Host pointers in and out; the call owns a stream and stream-ordered device buffers
 * (thread-safe, independent of any engine, no device-wide synchronisation).  consensus [cap] receives 0..3; n1, n2
 * [cap] int32 and q_top [cap] float64 come together or are all NULL; *out_len the length; CHIRON_ERR_OVERFLOW if cap is
 * too small (then *out_len = needed).  kernal: CHIRON_KERNAL_GLUE or _STICK.                                       */
chiron_status chiron_consensus_device(int32_t device_id, const uint8_t* bases, const int64_t* seg_off, int64_t n_seg,
                                      const double* seg_qs, int32_t kernal, uint8_t* consensus, int32_t* n1, int32_t* n2,
                                      double* q_top, int64_t cap, int64_t* out_len);

/* Host-side reader of the reference's raw-signal text format: chiron_input.py:527-539 read_signal() --
 * `f.read().split()` converted to float32 -- whitespace/newline separated numbers.  Each token is parsed as a
 * C double (like Python's float()) and then narrowed to float32, so the values equal numpy's conversion.
 * out holds up to cap values; *n_out receives the number parsed.  A token that is not a number ->
 * CHIRON_ERR_INVALID (the reference raises ValueError); more than cap values -> CHIRON_ERR_OVERFLOW.
 * Pure host code: callable without a GPU and from several threads at once (it does not touch Python). */
chiron_status chiron_parse_signal_text(const char* text, size_t len, float* out, size_t cap, size_t* n_out);

/* fast5 (HDF5) reader without libhdf5 / h5py: what chiron/utils/extract_sig_ref.py:149-193 (extract_file for single-read
 * files: the first group under /Raw/Reads; extract_file_v2 for multi-read files: one read per top-level group, sorted by
 * name) takes from a file -- raw signal, read_id attribute, reference FASTQ / FASTA if present.  Replaces, together with
 * chiron_input.py:541-555 read_signal_fast5, the extract -> `.signal` text -> read_signal round trip of `chiron call`
 * (SURVEY 8(f)1).  Host code (zlib for the deflate filter): no GPU, thread-safe, every handle owns its file image.
 * An unsupported or damaged file gives CHIRON_ERR_INVALID with the reason in chiron_last_error(); the caller logs and
 * skips it, like the reference (extract_sig_ref.py:97-117).                                                        */
typedef struct chiron_fast5 chiron_fast5;
chiron_status chiron_fast5_open(const char* path, chiron_fast5** out);
void chiron_fast5_close(chiron_fast5* f);
int32_t chiron_fast5_read_count(const chiron_fast5* f);
/* read i: suffix ("" for a single-read file, the read's group name in a multi-read file: the .signal name is
 * <file stem><suffix>, extract_sig_ref.py:128-144), read_id, number of samples, length of the reference text (0: none) */
chiron_status chiron_fast5_read_info(const chiron_fast5* f, int32_t i, char* suffix, size_t suffix_cap, char* read_id,
                                     size_t id_cap, int64_t* n_samples, int64_t* fastq_len);
/* the raw signal of read i as float32 (np.float32 of the DAC counts, chiron_input.py:536); reverse != 0 stores it
 * back to front (RNA: extract_sig_ref.py:165 / chiron_input.py:269-272) */
chiron_status chiron_fast5_signal(const chiron_fast5* f, int32_t i, float* out, int64_t cap, int32_t reverse);
chiron_status chiron_fast5_fastq(const chiron_fast5* f, int32_t i, char* out, int64_t cap);
/* extract_sig_ref.py:122-123: delimiter.join(str(v) for v in raw_signal) written to `path` for integer-valued samples
 * (what `chiron call` extracts: unit = False, entry.py:36); a non-integer sample is refused (CHIRON_ERR_INVALID). */
chiron_status chiron_write_signal_text(const char* path, const float* v, int64_t n, const char* delimiter);

/* The host side of `chiron call` on its direct fast5 path as ONE native call (ABI 7): reader threads (fast5 -> samples, raw/<name>.signal
 * and reference/<stem>_ref.fastq as extract_sig_ref.py:92-147 writes them, windows as rows of one zero-padded buffer at stride `jump`:
 * chiron_input.py:276-286), the CALLING thread packing batches across reads in file order (chiron_eval.py:321-334, seq_len rounded half
 * even :337), submitting them to the engine's slots and regrouping the compact decode per read (:403-446), finisher threads running
 * chiron_finish_read + meta/<name>.meta (:446-462, :176-242).  It replaces the Python thread pools of chiron_amd/eval.py:evaluation --
 * same files, byte for byte, except the timings inside meta/ -- for: fast5 input, bn_mode population (a partial last batch is submitted
 * as it is), host-side vote for every read; `.signal` text files are taken as well (name_root).  The folders raw/ reference/ result/
 * segments/ meta/ under `output` must exist (sub-folders of a recursive `.signal` input are created on demand).
 * null_engine != 0: no engine call is made (e may be NULL): collect() is replaced by a canned decode of ~44 bases per window -- the host
 * pipeline's own ceiling (tools/host_ceiling.py).  Unreadable files are skipped and reported in stats->messages (the reference logs and
 * skips them, extract_sig_ref.py:97-117); a failed engine call or file write ends the run with its status.                           */
typedef struct {
  int32_t batch_size, segment_len, jump, start;   /* FLAGS.batch_size / segment_len / jump / start                                    */
  int32_t beam;                                    /* 0 = greedy                                                                       */
  int32_t fastq, concise, rna, no_raw;             /* -e fastq; --concise; --mode rna (signal reversed, U for T); --no-raw             */
  int32_t n_threads;                               /* reader threads = finisher threads                                                */
  int32_t n_slots;                                 /* the engine's slots (chiron_engine_opts.n_slots)                                  */
  int32_t null_engine;
  double null_ratio;                               /* null engine only: segment_len / T                                                */
  const char* output;                              /* FLAGS.output                                                                     */
  const char* delimiter;                           /* of raw/<name>.signal ("\n": HEAD; NULL = "\n")                                   */
  const char* input_name;                          /* meta/<name>.meta: FLAGS.input, FLAGS.model                                       */
  const char* model_name;
  const char* name_root;                           /* `.signal` inputs (a path ending in ".signal" is parsed as text: chiron_input.py:527-539, and
                                                      nothing is written to raw/ or reference/): a read is named by its path relative to this
                                                      folder, sub-folders included (chiron_eval.py:277-293); NULL: by its file name          */
} chiron_pipeline_opts;
typedef struct {
  int64_t reads, reads_finished, windows, batches, consensus_bases, files_failed;
  double seconds;
  char messages[4096];                             /* one line per skipped file / first failure                                        */
} chiron_pipeline_stats;
chiron_status chiron_pipeline_run(chiron_engine* e, const char* const* fast5_paths, int64_t n_paths, const chiron_pipeline_opts* opts,
                                  chiron_pipeline_stats* stats);

/* CRC-32C (Castagnoli) of a byte range: the checksum TF's tensor-bundle checkpoints record per tensor
 * (BundleEntryProto.crc32c holds its masked form; tensor_bundle.cc verifies it in Saver.restore, chiron_eval.py:276).
 * Host code, used by the checkpoint reader.                                                                        */
chiron_status chiron_crc32c(const void* data, size_t len, uint32_t* out);

/* PCI address ("0000:c1:00.0", lower case as sysfs spells it) of HIP device `device_id`: what `chiron call --gpus N` needs to put
 * rank r on the cores of the NUMA node its GPU hangs off (/sys/bus/pci/devices/<address>/numa_node; chiron_amd/shard.py).
 * The reference has no counterpart: it is one process on one device (chiron_eval.py:255-262).  cap >= 16.            */
chiron_status chiron_device_pci_bus_id(int32_t device_id, char* out, size_t cap);

/* CTC loss and its gradient, chiron/chiron_model.py:50-75 loss(): tf.nn.ctc_loss(label, logits, seq_len, ctc_merge_repeated=True,
 * time_major=False, ignore_longer_outputs_than_inputs=True) per window (the mean, and the focal term fl_gamma, are left to the caller).
 * Classes A,C,G,T = 0..3 (chiron_input.py:710-730 base2ind), blank = 4 (the last class); labels are NOT collapsed beforehand
 * (preprocess_collapse_repeated=False), so a repeat needs a blank between its two frames.  loss = -log p(label | logits) with a
 * log-softmax over the 5 classes of every frame; frames t >= seq_len[b] are ignored and get a zero gradient.  The gradient is with
 * respect to the LOGITS (pre-softmax), as TF returns it: softmax(t,k) - posterior(t,k).
 * Rows with label_len > seq_len: loss 0, gradient 0 (skipped, ignore_longer_outputs_than_inputs).  Rows that fit by length but not
 * once every repeat has its blank (label_len + repeats > seq_len): loss +inf, gradient 0 (infeasible).  TF raises "Not enough time
 * for target transition sequence" there; a batch call cannot raise per row.  This rule is recalled TF behaviour, not a measurement
 * of TF.  label_len 0 is legal: the loss is -sum_t log softmax(t, blank).
 *
 * The recursions run in double (log space); the loss is rounded to float at the end.
 * Workspace: with CHIRON_CTC_WANT_GRAD the forward pass keeps alpha of every frame, in double, for the backward pass,
 *   bytes = batch * T * S_max * 8,   S_max = 2 * min(max_label_len, T) + 1,
 * and 0 bytes without it.  Host-only (no GPU needed).  CHIRON_ERR_OVERFLOW when T > CHIRON_CTC_MAX_T or max_label_len >
 * CHIRON_CTC_MAX_LABEL; within those bounds every workspace stays below 2^62 bytes and every offset the kernels form is 64-bit.
 *
 * Caller's memory.  This holds for every call below that takes a workspace, a tape or a device output buffer from its caller --
 * chiron_ctc_loss, chiron_rnn_train_forward / _backward, chiron_cnn_train_forward / _backward, chiron_align_pairs,
 * chiron_align_trace, chiron_align_infix, chiron_align_overlap, chiron_seed_reads, chiron_seed_candidates, chiron_ctc_align, chiron_ctc_score, chiron_demux_windows,
 * chiron_pileup, chiron_signal_levels, chiron_signal_refine, chiron_signal_locate, chiron_event_locate and chiron_signal_score; their own comments say "uninitialised" or name the size function and mean this:
 *   - workspace, tape and output buffers may hold anything on entry: the results do not depend on it (the library clears what it
 *     needs cleared, on the call's stream);
 *   - every element of every output is written, the rows and frames that carry no result included (frames past seq_len, skipped and
 *     infeasible rows, the pop_mean / pop_var slots of a gradient).  The two exceptions are stated where they apply: moments_out of
 *     chiron_cnn_train_forward (only the statistics' slots are written) and a failed pair's slice of chiron_align_trace's ops_out;
 *   - nothing outside the bytes that the call's *_workspace_size / *_train_sizes function names, and outside the outputs' own
 *     extents, is read or written: a caller may pack other data right behind a workspace of exactly that size.
 * tests/test_gpu_workspace.py holds every one of these calls to the three parts (chiron_signal_levels: tests/test_gpu_squiggle.py; chiron_signal_refine:
 * tests/test_gpu_refine.py; chiron_signal_locate: tests/test_gpu_locate.py; chiron_event_locate: tests/test_gpu_event_locate.py;
 * chiron_signal_score: tests/test_gpu_modcall.py; chiron_align_overlap: tests/test_gpu_overlap.py). */
#define CHIRON_CTC_WANT_GRAD 1u
#define CHIRON_CTC_TRUSTED 2u   /* chiron_ctc_loss: the caller has checked seq_len / labels / label_len: no read-back, no sync */
#define CHIRON_CTC_MAX_T 8192
#define CHIRON_CTC_MAX_LABEL (1 << 24)
chiron_status chiron_ctc_workspace_size(int32_t batch, int32_t T, int32_t max_label_len, uint32_t flags, size_t* bytes);

/* Stand-alone CTC loss (and, with CHIRON_CTC_WANT_GRAD, its gradient) for torch users: every operand is a device pointer on
 * device_id.  logits float32 [batch, T, 5]; seq_len int32 [batch]; labels int32 [batch, max_label_len] dense, padded; label_len
 * int32 [batch]; loss_out float32 [batch]; grad_out float32 [batch, T, 5] (written only with CHIRON_CTC_WANT_GRAD); workspace of
 * chiron_ctc_workspace_size bytes (NULL without the flag; "Caller's memory" above).  Asynchronous on `stream` (a hipStream_t; NULL = the null stream), with
 * one exception: seq_len, labels and label_len are first read back on `stream` (a small synchronous copy) and checked, so that an
 * argument error returns CHIRON_ERR_INVALID before anything is launched: a label outside 0..3, label_len < 0 or > max_label_len,
 * seq_len < 0 or > T, batch < 0.  With CHIRON_CTC_TRUSTED that read-back is skipped and the call is fully asynchronous; the
 * kernels then clamp seq_len to 0..T and label_len to 0..max_label_len and read labels modulo 4 (memory-safe, but the result of
 * an unchecked bad argument is unspecified).  Deterministic: the same bits run to run.                                                       */
chiron_status chiron_ctc_loss(int32_t device_id, const float* logits, const int32_t* seq_len, const int32_t* labels,
                              const int32_t* label_len, int32_t batch, int32_t T, int32_t max_label_len, uint32_t flags,
                              float* loss_out, float* grad_out, void* workspace, void* stream);

/* Score the slot's most recent COLLECTED batch against known bases, as the reference's validation does: the CTC loss above on the
 * batch's device logits and seq_len (chiron_model.py:50-75, fl_gamma and the mean left to the caller) and
 * tf.edit_distance(decoded, label, normalize=True) (chiron_model.py:101-132) of the batch's device decode -- the SparseTensor
 * (indices, values) every decode path leaves on the device (greedy, beam, chiron_engine_decode, CHIRON_COMPACT_DECODE) -- against
 * the labels: Levenshtein distance / truth length; an empty truth gives 0 against an empty decode and +inf otherwise (recalled TF
 * behaviour).  labels int32 [batch, max_label_len] and label_len [batch] are HOST arrays; loss_out, edit_out [batch] float32 and
 * status_out [batch] int32 (0 = scored, 1 = skipped, 2 = infeasible; see chiron_ctc_workspace_size) are host arrays too.  Runs on
 * the slot's stream with no host round trip of logits or decode and synchronises that stream before returning.  The engine's label
 * and workspace buffers grow on demand and are freed by chiron_engine_destroy.  flags: 0 (reserved).  CHIRON_ERR_STATE when no
 * batch has been collected on the slot, the slot holds an uncollected batch, or batch differs from the collected batch's size.   */
chiron_status chiron_engine_score(chiron_engine* e, int32_t slot, const int32_t* labels, const int32_t* label_len, int32_t batch,
                                  int32_t max_label_len, uint32_t flags, float* loss_out, float* edit_out, int32_t* status_out);

/* Training seam of the recurrent stack and the FC head: what chiron_rcnn_train.py:99-109 (sess.run([net.ctc_loss, net.step])) needs
 * between the CNN's feature tensor and the logits, for the variables of rnn.py:20-97 (DNA), :99-174 (RNA) and the head :72-96.  The
 * CNN stays frozen; fp32 only; hidden 100 and 5 classes (CHIRON_ERR_INVALID otherwise).  Optimizer and loss stay with the caller
 * (chiron_model.py:77-99 train_opt; chiron_ctc_loss above gives d loss / d logits).
 *
 * The trainable parameter vector IS a slice of the weight blob of chiron_weights_size, in that layout: from the first
 * lstm_cell/kernel to rnn_fnn_layer/bias_class.  chiron_rnn_params_range returns where it starts and how long it is (floats);
 * gradients come back in the same layout.  Host-only.                                                                            */
chiron_status chiron_rnn_params_range(const chiron_model_desc* desc, size_t* first_float, size_t* n_floats);

/* Bytes of the tape (what the forward pass keeps for the backward pass: the transposed features, every layer's output, and per
 * step, row and direction the four activated gates and the cell state) and of the workspace (x-projections, gate derivatives,
 * dh buffers, split-K partial sums) for one batch of `batch` windows of T frames.  Both grow linearly in the batch rounded up to
 * 16 rows.  Host-only (no GPU needed).  CHIRON_ERR_INVALID: batch < 1, T < 1, unsupported topology.  CHIRON_ERR_OVERFLOW: T >
 * CHIRON_CTC_MAX_T, batch > 2^20, or T * roundup(batch, 16) > 128 * 65535 = 8 388 480 rows (the GEMMs' 128-row tiles lie along a
 * grid's y extent, and the kernels index at most 2^24 rows); within those bounds every offset the kernels form is 64-bit.  The
 * launchers below make the same checks.                                                                                           */
chiron_status chiron_rnn_train_sizes(const chiron_model_desc* desc, int32_t batch, int32_t T, size_t* tape_bytes, size_t* workspace_bytes);

/* Forward with a tape (rnn.py:20-174 + :72-96 in training): logits_out [batch, T, 5] from features [batch, T, C] (the tensor of
 * chiron_engine_features) and seq_len int32 [batch], with the semantics of the inference layers: gate order i, j, f, o; forget bias
 * +1.0; frames t >= seq_len[b] emit 0 and carry the state; the backward direction runs over the first seq_len[b] frames reversed
 * (seq_len is clamped to 0..T).  params: the slice of chiron_rnn_params_range.  Every pointer is device memory on device_id; tape
 * and workspace of chiron_rnn_train_sizes bytes, uninitialised ("Caller's memory" above).  Asynchronous on `stream` (a hipStream_t; NULL = the null stream);
 * argument errors are reported before anything is launched.                                                                       */
chiron_status chiron_rnn_train_forward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* features,
                                       const int32_t* seq_len, int32_t batch, int32_t T, float* logits_out, void* tape, void* workspace,
                                       void* stream);

/* Backward of the call above (tf.gradients behind opt.minimize, chiron_rcnn_train.py:52-62): from dlogits [batch, T, 5] and the
 * tape that chiron_rnn_train_forward filled for the SAME params, features, seq_len, batch and T, dparams_out receives d loss / d
 * params in the layout of the slice, and dfeatures_out [batch, T, C] (may be NULL) d loss / d features: exactly 0 at frames t >=
 * seq_len[b].  Every reduction over the T * batch rows goes through per-slice partial sums in the workspace and a second pass in
 * slice order, never through float atomics: the same bits run to run.  The workspace may be the forward's (its content is not
 * needed).  Asynchronous on `stream`; argument errors are reported before anything is launched.                                   */
chiron_status chiron_rnn_train_backward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* features,
                                        const int32_t* seq_len, const float* dlogits, int32_t batch, int32_t T, const void* tape,
                                        void* workspace, float* dparams_out, float* dfeatures_out, void* stream);

/* The device pointer behind chiron_engine_features (getcnnfeature, cnn.py:334-371): float32 [batch, T, C] of the batch most recently
 * run on an idle slot, valid until the next submit on that slot; written on the slot's stream, which chiron_engine_collect has
 * synchronised.  fp32 engines only (CHIRON_ERR_INVALID otherwise); CHIRON_ERR_STATE as chiron_engine_features.  The frozen CNN's
 * output reaches the trainer above without a host round trip.                                                                     */
chiron_status chiron_engine_device_features(chiron_engine* e, int32_t slot, const float** ptr, int32_t* batch, int32_t* channels);

/* Training seam of the CNN: what chiron_rcnn_train.py:30-136 needs between the signal and the feature tensor, for every variable of
 * cnn.py that ModelSpec describes (the optional stem conv_layer/conv1 and the residual blocks: branch1/conv1, branch2/conv2a,
 * conv2b, conv2c with their BN sites).  fp32 only.  Batch normalisation ALWAYS uses the batch's own moments here, whatever
 * desc->bn_mode says: biased variance over all batch * T_site positions of a site, epsilon float32(1e-5) (simple_global_bn,
 * cnn.py:166-188; the training=True branch of batchnorm, cnn.py:151-158); the gradient flows through mean and variance.  The CNN
 * does not see seq_len: the zero-padded tail of a short window takes part in the moments, as in the reference.
 *
 * The trainable parameter vector is the CNN section of the weight blob of chiron_weights_size, in that layout: everything before
 * the first lstm_cell/kernel.  Every BN site has its four slots scale, offset, pop_mean, pop_var.  chiron_cnn_params_range returns
 * where the section starts (0) and how long it is (floats); together with chiron_rnn_params_range it tiles the blob.  Host-only. */
chiron_status chiron_cnn_params_range(const chiron_model_desc* desc, size_t* first_float, size_t* n_floats);

/* Bytes of the tape (every BN site's convolution output and statistics, every ReLU output) and of the workspace (four
 * activation-sized buffers, per-slice partial sums) for one batch of `batch` windows of segment_len samples.  Both grow linearly
 * in the batch apart from a term of at most a few MB for the partial sums.  Host-only.  CHIRON_ERR_INVALID: batch < 1,
 * segment_len < 1, unsupported topology (more than 2048 channels).  CHIRON_ERR_OVERFLOW: batch > 2^20, batch * segment_len > 2^24
 * rows, or more than CHIRON_CTC_MAX_T output frames; within those bounds every offset the kernels form is 64-bit.  The launchers
 * below make the same checks.                                                                                                    */
chiron_status chiron_cnn_train_sizes(const chiron_model_desc* desc, int32_t batch, int32_t segment_len, size_t* tape_bytes,
                                     size_t* workspace_bytes);

/* Where the tape keeps ReLU output number `index` (network order: the stem's when there is one, then per block conv2a's, conv2b's
 * and the block's output): float offset into the tape, frames per window and channels of the [batch, frames, channels] tensor.  The
 * rest of the tape is opaque.  The sign pattern of these tensors is the set of ReLU masks the backward uses, which is what a check
 * of the gradients against a smooth reference needs.  Host-only.  CHIRON_ERR_INVALID: index out of range; otherwise the statuses
 * of chiron_cnn_train_sizes.                                                                                                    */
chiron_status chiron_cnn_train_tape_relu(const chiron_model_desc* desc, int32_t batch, int32_t segment_len, int32_t index,
                                         size_t* offset_floats, int32_t* frames, int32_t* channels);

/* Forward with a tape: features_out [batch, T, C] (the layout chiron_rnn_train_forward takes) from signal [batch, segment_len].
 * params: the section of chiron_cnn_params_range; its pop_mean / pop_var slots are not read.  moments_out has the layout of
 * params; only the pop_mean / pop_var slots are written: each site's batch mean and biased variance (the moving averages are the
 * caller's arithmetic, cnn.py:153-156).  Every pointer is device memory on device_id, 16-byte aligned; tape and workspace of
 * chiron_cnn_train_sizes bytes, uninitialised ("Caller's memory" above).  Asynchronous on `stream` (a hipStream_t; NULL = the null stream); argument errors
 * are reported before anything is launched.                                                                                      */
chiron_status chiron_cnn_train_forward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* signal,
                                       int32_t batch, int32_t segment_len, float* features_out, float* moments_out, void* tape,
                                       void* workspace, void* stream);

/* Backward of the call above: from dfeatures [batch, T, C] (dfeatures_out of chiron_rnn_train_backward) and the tape that
 * chiron_cnn_train_forward filled for the SAME params, signal, batch and segment_len, dparams_out receives d loss / d params in
 * the layout of the section; the pop_mean / pop_var slots receive exactly 0.  No gradient with respect to the signal is produced.
 * Every reduction over rows (BN sums, weight gradients) goes through per-slice partial sums whose slice count depends on the
 * shape alone and a second pass in slice order, never through float atomics: the same bits run to run.  The workspace may be
 * the forward's (its content is not needed).  Asynchronous on `stream`; argument errors are reported before anything is launched. */
chiron_status chiron_cnn_train_backward(int32_t device_id, const chiron_model_desc* desc, const float* params, const float* signal,
                                        const float* dfeatures, int32_t batch, int32_t segment_len, const void* tape, void* workspace,
                                        float* dparams_out, void* stream);

/* Read-level assessment: global alignment of a basecalled read against the sequence it should have been, unit costs, for the
 * identity / mismatch / insertion / deletion rates a basecaller is judged by (the arithmetic behind the reference's
 * utils/assess.sh; references are per-read sequences, and chiron_align_infix below cuts them out of a genome).  Per pair (read a of n bases,
 * reference b of m bases) the result is (E, M): E the Levenshtein distance, M the largest number of matching columns over all
 * alignments of cost E (minimise E, then maximise M).  The operation counts follow without a traceback: mismatches X = n + m - 2M
 * - E, insertions I = n - M - X (read bases the reference lacks), deletions D = m - M - X.  Codes 0..3 = A, C, G, T (U is T); code
 * 4 matches nothing, not even itself.  Empty sequences are legal: E = max(n, m), M = 0.
 *
 * One workgroup aligns one pair inside a band of diagonals j - i in [min(0, m-n) - w, max(0, m-n) + w], w = CHIRON_ALIGN_BAND0
 * at first.  A path that leaves the band costs at least 2(w+1) + |m-n|, so a banded result with E <= 2w + 1 + |m-n| is exact in E
 * and in M; otherwise the workgroup doubles w and repeats, up to the full table.  band_out is the w that was accepted.  The
 * result is exact, deterministic, and independent of what else is in the batch.
 *
 * Workspace (device memory): the packed codes, the per-pair records and results, and -- when a table of 2 * max_len + 1 diagonals
 * is wider than the CHIRON_ALIGN_LDS_SLOTS the kernel keeps on chip -- one row of 2 * max_len + 2 64-bit cells for each of at most
 * CHIRON_ALIGN_MAX_GROUPS workgroups.  max_len: the longest sequence of the call (a larger value is fine).  Host-only.
 * CHIRON_ERR_INVALID: pairs < 0, max_len < 0.  CHIRON_ERR_OVERFLOW: max_len > CHIRON_ALIGN_MAX_LEN or pairs > 2^24; within those
 * bounds every offset the kernel forms is 64-bit and every count fits 32 bits.                                                  */
#define CHIRON_ALIGN_MAX_LEN (1 << 17)
#define CHIRON_ALIGN_BAND0 256
#define CHIRON_ALIGN_THREADS 256      /* cells of one anti-diagonal a workgroup updates per pass                                  */
#define CHIRON_ALIGN_LDS_SLOTS 4096   /* widest band (diagonals) whose cells stay in LDS; wider bands use the workspace row        */
#define CHIRON_ALIGN_MAX_GROUPS 2048  /* workgroups of one launch; pair p runs on workgroup p mod the launch's group count        */
chiron_status chiron_align_workspace_size(int64_t pairs, int64_t max_len, size_t* bytes);

/* Align `pairs` pairs in one launch.  codes: HOST bytes; pair p's read is codes[read_off[p] .. read_off[p+1]) and its reference
 * codes[ref_off[p] .. ref_off[p+1]); read_off and ref_off are HOST int64 [pairs + 1], non-negative and non-decreasing (the two
 * may interleave in any way; typically all reads, then all references).  edit_out, match_out, band_out: HOST int32 [pairs].
 * workspace: device memory on device_id of chiron_align_workspace_size(pairs, longest sequence) bytes ("Caller's memory" above).  flags: 0 (reserved).
 * Runs on `stream` (a hipStream_t; NULL = the null stream) and synchronises it before returning.  CHIRON_ERR_INVALID for a bad
 * offset or a code above 4, CHIRON_ERR_OVERFLOW for a sequence longer than CHIRON_ALIGN_MAX_LEN, both before anything is copied
 * or launched.  pairs == 0 is a no-op.                                                                                         */
chiron_status chiron_align_pairs(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const int64_t* ref_off, int64_t pairs,
                                 uint32_t flags, int32_t* edit_out, int32_t* match_out, int32_t* band_out, void* workspace, void* stream);

/* Alignment traceback: the canonical optimal alignment of a pair whose (E, M) is known, one byte per column: 0 '=' (match),
 * 1 'X' (mismatch), 2 'I' (a read base without a reference base), 3 'D' (a reference base without a read base).  Codes and the
 * match rule are those of chiron_align_pairs.  Among the global alignments with the smallest E and then the largest M, the
 * canonical one is the one whose column string, read from the LAST column to the first, is smallest under the order diagonal
 * ('=' or 'X') < 'I' < 'D'.  Cell by cell: walking back from (n, m), each cell takes the first admissible predecessor in the
 * order diagonal, up, left, where p is admissible for c when K(p) + cost(p -> c) = K(c) on the keys K = E * 2^32 - M.  Gaps in a
 * repeat are therefore left-aligned.  It is a property of the inputs.  An infix alignment is traced as the read against the
 * window's substring [s, e) that chiron_align_infix returned.
 *
 * The sweep runs once, at the half-width the known cost allows: a path that touches diagonal max(0, m-n) + x, x >= 1, costs at
 * least 2x + |m-n|, so every alignment of cost E lies on the diagonals [min(0, m-n) - w, max(0, m-n) + w], w = (E - |m-n|) / 2
 * (rounded down).  The back-pointers cover that band only: one row per anti-diagonal, 2 bits a cell, four cells a byte.
 *
 * The pair-size helper (host-only) gives one pair's back-pointer bytes and its band in diagonals from (n, m, edit), so a caller can
 * plan batches against a memory budget.  CHIRON_ERR_INVALID: a negative length, edit < |m-n| or edit > max(n, m);
 * CHIRON_ERR_OVERFLOW: a length past CHIRON_ALIGN_MAX_LEN.
 *
 * Workspace (device memory): the per-pair records and statuses, the packed codes and the columns (2 * max_len bytes a pair each),
 * backpointer_bytes of back-pointers (the sum over the call's pairs) and -- when max_band, the call's widest band in diagonals,
 * passes CHIRON_ALIGN_LDS_SLOTS -- one row of max_band + 1 64-bit cells for each of at most CHIRON_ALIGN_MAX_GROUPS workgroups.
 * Larger values of any argument are fine.  Host-only.  CHIRON_ERR_INVALID: a negative argument.  CHIRON_ERR_OVERFLOW: max_len >
 * CHIRON_ALIGN_MAX_LEN, pairs > 2^24 or backpointer_bytes > 2^46; within those bounds every offset the kernel forms is 64-bit.    */
chiron_status chiron_align_trace_pair_size(int64_t n, int64_t m, int64_t edit, int64_t* backpointer_bytes, int64_t* band);
chiron_status chiron_align_trace_workspace_size(int64_t pairs, int64_t backpointer_bytes, int64_t max_len, int64_t max_band, size_t* bytes);

/* Trace `pairs` pairs in one launch.  codes, read_off, ref_off: as for chiron_align_pairs.  edit_in, match_in: HOST int32 [pairs],
 * the pair's (E, M) as chiron_align_pairs or chiron_align_infix returned it.  ops_off: HOST int64 [pairs + 1], non-negative; pair
 * p's columns are ops_out[ops_off[p] .. ops_off[p+1]), first column first, and ops_off[p+1] - ops_off[p] must be the pair's
 * column count n + m - M - X = E + M.  status_out: HOST int32 [pairs]: 0 traced; 1 the kernel's own (E, M) of the pair is not
 * the one passed in, and the pair's slice of ops_out is left untouched (the other pairs are unaffected).  workspace: device memory
 * on device_id of chiron_align_trace_workspace_size bytes for the call's pairs ("Caller's memory" above).  flags: 0 (reserved).  Runs on `stream` (a
 * hipStream_t; NULL = the null stream) and synchronises it before returning.  CHIRON_ERR_INVALID for a bad offset, a code above
 * 4, edit < |m-n|, edit > max(n, m), a match count the lengths and edit rule out, or an ops_off that disagrees with the column
 * count; CHIRON_ERR_OVERFLOW for a sequence longer than CHIRON_ALIGN_MAX_LEN; all before anything is copied or launched.
 * pairs == 0 is a no-op.  Empty sequences are legal: all 'D' or all 'I'.                                                         */
chiron_status chiron_align_trace(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const int64_t* ref_off, int64_t pairs,
                                 const int32_t* edit_in, const int32_t* match_in, const int64_t* ops_off, uint32_t flags, uint8_t* ops_out,
                                 int32_t* status_out, void* workspace, void* stream);

/* Read mapping: infix (semi-global) alignment of a read against a genome window, unit costs, same codes as chiron_align_pairs.
 * Per pair (read a of n bases, window b of m bases), over every substring b[s:e), 0 <= s <= e <= m, and every global alignment
 * of a against it, the result is the tuple (E, M, s, e) that is smallest in this order: smallest edit cost E, then largest
 * number of matching columns M, then smallest s, then smallest e.  It is a property of the inputs, not of a tie order inside the
 * kernel.  Empty inputs are legal: n = 0 gives (0, 0, 0, 0), m = 0 gives (n, 0, 0, 0).  X, I, D of the chosen alignment follow as
 * for chiron_align_pairs with the reference length e - s.
 *
 * One workgroup aligns one pair; a cell carries (E, -M, s) in one 64-bit key E * 2^40 - M * 2^20 + s, which is why a read has at
 * most CHIRON_INFIX_MAX_READ and a window at most CHIRON_INFIX_MAX_WINDOW bases.  The sweep covers the diagonals j - i in
 * [min(0, m-n) - w, max(0, m-n) + w], w = band0 at first.  An alignment starts on a diagonal s >= 0 and ends on one <= m - n, and
 * only a gap changes the diagonal, so one that touches a diagonal outside the band -- one that starts above it included -- costs
 * at least w + 1: a banded result with E <= w is exact in all four values for the whole window.  (Not the 2w + 1 + |m-n| of
 * chiron_align_pairs: the ends are free here.)  Otherwise the workgroup doubles w and repeats, up to the full table, which is
 * always accepted.  band_out is the w that was accepted.  band0 = 0: the full table at once, band_out = 0.  The result is exact,
 * deterministic, and independent of what else is in the batch.
 *
 * Workspace (device memory): the packed codes, the per-pair records and results, and -- when a table of max_read + max_window + 1
 * diagonals is wider than the CHIRON_INFIX_LDS_SLOTS the kernel keeps on chip -- one row of that many 64-bit cells (plus one) for
 * each of at most CHIRON_INFIX_MAX_GROUPS workgroups.  max_read, max_window: the longest of the call (larger values are fine).
 * Host-only.  CHIRON_ERR_INVALID: a negative argument.  CHIRON_ERR_OVERFLOW: max_read > CHIRON_INFIX_MAX_READ, max_window >
 * CHIRON_INFIX_MAX_WINDOW or pairs > 2^24; within those bounds every offset the kernel forms is 64-bit.                          */
#define CHIRON_INFIX_MAX_READ (1 << 17)
#define CHIRON_INFIX_MAX_WINDOW ((1 << 20) - 1)
#define CHIRON_INFIX_BAND0 256        /* the band0 the `map` command passes                                                       */
#define CHIRON_INFIX_THREADS 256      /* cells of one anti-diagonal a workgroup updates per pass                                  */
#define CHIRON_INFIX_LDS_SLOTS 4096   /* widest band (diagonals) whose cells stay in LDS; wider bands use the workspace row        */
#define CHIRON_INFIX_MAX_GROUPS 2048  /* workgroups of one launch; pair p runs on workgroup p mod the launch's group count        */
chiron_status chiron_align_infix_workspace_size(int64_t pairs, int64_t max_read, int64_t max_window, size_t* bytes);

/* Align `pairs` pairs in one launch.  codes: HOST bytes; pair p's read is codes[read_off[p] .. read_off[p+1]) and its window
 * codes[win_off[p] .. win_off[p+1]); read_off and win_off are HOST int64 [pairs + 1], non-negative and non-decreasing.  edit_out,
 * match_out, start_out, end_out, band_out: HOST int32 [pairs]; start and end are offsets into the pair's window.  workspace:
 * device memory on device_id of chiron_align_infix_workspace_size(pairs, longest read, longest window) bytes ("Caller's memory" above).  flags: 0
 * (reserved).  Runs on `stream` (a hipStream_t; NULL = the null stream) and synchronises it before returning.
 * CHIRON_ERR_INVALID for a bad offset, a code above 4 or band0 < 0, CHIRON_ERR_OVERFLOW for a read or window past its limit, all
 * before anything is copied or launched.  pairs == 0 is a no-op.                                                                */
chiron_status chiron_align_infix(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const int64_t* win_off, int64_t pairs,
                                 int32_t band0, uint32_t flags, int32_t* edit_out, int32_t* match_out, int32_t* start_out,
                                 int32_t* end_out, int32_t* band_out, void* workspace, void* stream);

/* Read-to-read overlaps: dovetail alignment of two reads -- a suffix of one against a prefix of the other, containment as the
 * limiting case -- inside a band of diagonals the caller gives.  Same codes as chiron_align_pairs (4 matches nothing).
 *
 * Read a has n bases and read b has m.  A path runs through the (n+1) x (m+1) table by diagonal, down and right moves; it STARTS on
 * row 0 or on column 0 and ENDS on row n or on column m, and every cell of it lies on a diagonal d = j - i of [dlo, dhi].  Its
 * cost is 2 E - M: M counts the diagonal moves on equal codes below 4, E every other move.  (Under unit cost the empty overlap
 * would always win; the score M - 2 E rises along any stretch of identity above 2/3.)  A boundary cell is named by its diagonal
 * shifted by n: a start (0, j) is s = j + n and a start (i, 0) is s = n - i; an end (n, j) is e = j and an end (i, m) is
 * e = m - i + n; a corner has one value either way.  The result of a pair is the tuple (cost, M, s, e) that is smallest in this
 * order over all paths in the band: smallest cost, then largest M, then smallest s, then smallest e.  It is a property of the
 * inputs, not of a tie order inside the kernel, and E = (cost + M) / 2.
 *
 * THE BAND IS PART OF THE DEFINITION, not an accelerator with a certificate as in chiron_align_pairs and chiron_align_infix: an
 * overlap on a diagonal outside it (a repeat) is another path, which nothing computed inside the band can exclude.  The kernel
 * never widens; chiron_amd/overlap.py owns the rule that does.  The band is clipped to the table's diagonals [-n, m] first, which
 * then always holds a boundary start; a band that is empty after clipping is refused.  The empty path at a corner, (0, m) on
 * diagonal m or (n, 0) on diagonal -n, costs 0, so the cost is never positive while the band holds one of those two diagonals; a
 * band that holds neither has no empty path (for n, m > 0) and its cost may be positive.  n = 0 or m = 0 gives cost 0 and M 0 at
 * the smallest s (= e) of the band.
 *
 * One workgroup of CHIRON_ALIGN_THREADS threads aligns one pair, pair p on workgroup p mod the group count (at most
 * CHIRON_ALIGN_MAX_GROUPS), by the banded anti-diagonal sweep of chiron_align_pairs under another cell policy; a cell carries
 * (cost, -M, start) in one signed 64-bit key cost * 2^40 - M * 2^20 + (start diagonal + 2^17), exact while a read has at most
 * CHIRON_OVERLAP_MAX_READ bases: M and the biased start stay below 2^20 and |cost| below 2^20.  The result is exact,
 * deterministic, and independent of what else is in the call.
 *
 * Workspace (device memory), each part rounded up to 256 bytes: 32 bytes and five int32 a pair, total_bases bytes of codes, and --
 * when max_band, the widest clipped band of the call in diagonals, is above the CHIRON_ALIGN_LDS_SLOTS the kernel keeps on chip --
 * one row of max_band 64-bit cells for each of min(pairs, CHIRON_ALIGN_MAX_GROUPS) workgroups.  Larger values of any argument
 * are fine.  Host-only.  CHIRON_ERR_INVALID: a negative argument.  CHIRON_ERR_OVERFLOW: pairs or reads > 2^24, total_bases >
 * reads * CHIRON_OVERLAP_MAX_READ, max_band > 2 * CHIRON_OVERLAP_MAX_READ + 1; within those bounds every offset the kernel forms
 * is 64-bit.                                                                                                                     */
#define CHIRON_OVERLAP_MAX_READ (1 << 17)
chiron_status chiron_align_overlap_workspace_size(int64_t reads, int64_t total_bases, int64_t pairs, int64_t max_band, size_t* bytes);

/* Align `pairs` pairs of the call's `reads` reads in one launch.  codes: HOST bytes; read r is codes[read_off[r] .. read_off[r+1]);
 * read_off is HOST int64 [reads + 1], non-negative and non-decreasing; the reads are copied once however many pairs name them.
 * pair_a, pair_b (read indices), dlo, dhi: HOST int32 [pairs]; pair p aligns read pair_a[p] as a against read pair_b[p] as b on
 * the diagonals dlo[p] .. dhi[p], both ends included, clipped to the table.  out: HOST int32 [pairs][5]: cost, M, s, e and a
 * status that is 0 in every result this call returns.  workspace: device memory on device_id of at least the size function's
 * bytes for (reads, read_off[reads] - read_off[0], pairs, the widest clipped band) ("Caller's memory" above); workspace_bytes says
 * how many it has.  flags: 0 (reserved).  Runs overlap_kernel on `stream` (a hipStream_t; NULL = the null stream) and synchronises
 * it before returning.  CHIRON_ERR_INVALID: unknown flags, a negative count, a null array that is needed, a negative or
 * decreasing offset, a code above 4, a read index outside 0 .. reads - 1, a band that is empty after clipping, a workspace smaller
 * than needed.  CHIRON_ERR_OVERFLOW: a read above CHIRON_OVERLAP_MAX_READ bases (the key's limit), pairs or reads > 2^24.  All of
 * it before anything is copied or launched, and `out` is written only by a call that returns CHIRON_OK.  pairs == 0 touches no
 * device and writes nothing.                                                                                                     */
chiron_status chiron_align_overlap(int32_t device_id, const uint8_t* codes, const int64_t* read_off, int64_t reads, const int32_t* pair_a,
                                   const int32_t* pair_b, const int32_t* dlo, const int32_t* dhi, int64_t pairs, int32_t* out,
                                   void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/* Seeding of the read mapper: where in a genome each read probably lies, from k-mer votes.  The index is the genome's k-mers of
 * k = CHIRON_SEED_K bases, 2 bits a base with the first base highest, sorted by value: idx_val[i] the value, idx_pos[i] the
 * position of the k-mer's first base in the (concatenated) genome, 0 <= idx_pos[i] <= genome_len - k; which k-mers it holds is the
 * caller's choice.  Reads are codes 0..4.  Each read of n bases is scored as given (strand 0) and as its reverse complement
 * (strand 1, the complement of code c < 4 is 3 - c); a k-mer that holds a code above 3 is skipped.  A hit of the k-mer at read
 * position r on an index entry with position g votes for the diagonal delta = g - r, in bin floor(delta / CHIRON_SEED_BIN).  The
 * score of a bin that holds a hit is its count plus the count of the next bin up.  The best score over both strands wins, ties to
 * strand 0, then to the smaller bin beta: that score is votes_out and the strand strand_out.  second_out is the larger of the
 * other strand's best score and the best score of a bin of the winning strand more than n / 256 + 2 bins from beta (0 without
 * either).  The candidate (delta_out, g_out) is the hit of rank (votes - 1) / 2, counted from 0, among the hits of bins beta and
 * beta + 1 of the winning strand ordered by (delta, g).  Without a hit votes_out and second_out are 0, strand_out is 0 and
 * delta_out and g_out carry no meaning.  Every value is an integer sum, a maximum over a total order or a rank, so the result is
 * a property of the inputs, and a read's result depends on that read alone.
 *
 * One workgroup of CHIRON_SEED_THREADS per read, read q on workgroup q mod the launch's group count (at most
 * CHIRON_SEED_MAX_GROUPS); each k-mer is looked up once by binary search, the bins are counted with int32 atomic adds into a
 * dense histogram per workgroup and strand, and the median is found by counting, not sorting (csrc/seed.hip).
 *
 * Workspace (device memory), each part rounded up to 256 bytes: the index (8 n_index bytes), total_bases + 1 bytes of codes, 16
 * bytes of record and 20 of results a read, and for each of min(reads, CHIRON_SEED_MAX_GROUPS) workgroups 16 max_read bytes of
 * looked-up k-mers and 8 ((genome_len + max_read rounded up to 256) / 256 + 2) bytes of counters.  Larger values of any argument
 * are fine.  Host-only.  CHIRON_ERR_INVALID: a negative argument.  CHIRON_ERR_OVERFLOW: reads > 2^24, max_read >
 * CHIRON_INFIX_MAX_READ, genome_len > CHIRON_SEED_MAX_GENOME (which keeps every delta and g in 32 bits with room for a read on
 * either side), n_index > 2^31 - 1, total_bases > reads * CHIRON_INFIX_MAX_READ.                                                  */
#define CHIRON_SEED_K 15
#define CHIRON_SEED_BIN 256
#define CHIRON_SEED_THREADS 256
#define CHIRON_SEED_MAX_GROUPS 2048
#define CHIRON_SEED_MAX_GENOME 0x7FFC0000   /* 2^31 - 2^18 */
chiron_status chiron_seed_workspace_size(int64_t n_index, int64_t genome_len, int64_t reads, int64_t max_read, int64_t total_bases,
                                         size_t* bytes);

/* Seed `reads` reads in one launch.  idx_val (uint32) and idx_pos (int32): HOST [n_index], as above.  codes: HOST bytes; read q is
 * codes[read_off[q] .. read_off[q+1]); read_off is HOST int64 [reads + 1], non-negative and non-decreasing.  votes_out,
 * second_out, strand_out (0 forward, 1 reverse): HOST int32 [reads]; delta_out, g_out: HOST int64 [reads].  workspace: device
 * memory on device_id of chiron_seed_workspace_size(n_index, genome_len, reads, longest read, sum of the reads) bytes ("Caller's memory" above).  flags: 0
 * (reserved).  The call keeps no state: it copies the index and the reads in, runs on `stream` (a hipStream_t; NULL = the null
 * stream) and synchronises it before returning.  CHIRON_ERR_INVALID for a null operand, unknown flags, a negative count, a bad
 * offset, a code above 4, an index that is not sorted or holds a position outside 0 .. genome_len - k; CHIRON_ERR_OVERFLOW past
 * the limits of the size function; all before anything is copied or launched.  reads == 0 is a no-op; n_index == 0 gives 0 votes
 * for every read and touches no device.  CHIRON_ERR_STATE if the kernel finds its own counters inconsistent.                    */
chiron_status chiron_seed_reads(int32_t device_id, const uint32_t* idx_val, const int32_t* idx_pos, int64_t n_index, int64_t genome_len,
                                const uint8_t* codes, const int64_t* read_off, int64_t reads, uint32_t flags, int32_t* votes_out,
                                int32_t* second_out, int32_t* strand_out, int64_t* delta_out, int64_t* g_out, void* workspace, void* stream);

/* Up to max_cand candidates a read instead of one, equal to map.vote_top (chiron_amd/map.py).  Bins, scores and strands are those
 * of chiron_seed_reads.  The picks are made greedily: among the (strand, bin) pairs that hold a hit and are not suppressed, the
 * largest score, ties to strand 0, then to the smaller bin; the picking stops when nothing is left, when that score is below
 * min_score, or after max_cand picks.  A pick at bin beta suppresses the bins b of its own strand with |b - beta| <= n / 256 + 2
 * (the complement of second_out's "far" rule, so pick 0 is chiron_seed_reads' candidate and pick 1's votes are its second_out).
 * Each pick's (delta, g) is the hit of rank (votes - 1) / 2 among the hits of bins beta and beta + 1 ordered by (delta, g).
 *
 * count_out: HOST int32 [reads], the number of picks; votes_out, strand_out: HOST int32 and delta_out, g_out: HOST int64, each
 * [reads][max_cand], pick c of read q at q * max_cand + c, zeros from count_out[q] on.  Everything else is as for
 * chiron_seed_reads, refusals included, with CHIRON_ERR_INVALID also for max_cand outside 1 .. CHIRON_SEED_MAX_CANDIDATES or
 * min_score < 1.  One launch: the k-mers are looked up and counted once a read, each pick replays the hits (csrc/seed.hip).
 * Workspace: that of chiron_seed_workspace_size with 4 + 16 max_cand bytes of results a read in place of 20.                    */
#define CHIRON_SEED_MAX_CANDIDATES 8
chiron_status chiron_seed_candidates_workspace_size(int64_t n_index, int64_t genome_len, int64_t reads, int64_t max_read, int64_t total_bases,
                                                    int32_t max_cand, size_t* bytes);
chiron_status chiron_seed_candidates(int32_t device_id, const uint32_t* idx_val, const int32_t* idx_pos, int64_t n_index, int64_t genome_len,
                                     const uint8_t* codes, const int64_t* read_off, int64_t reads, int32_t max_cand, int32_t min_score,
                                     uint32_t flags, int32_t* count_out, int32_t* votes_out, int32_t* strand_out, int64_t* delta_out,
                                     int64_t* g_out, void* workspace, void* stream);

/* CTC forced alignment: given a read's frame scores and the bases it is known to have, the best monotone assignment of frames
 * to bases (what a resquiggler gives the reference project; here from the model's own logits).  Read r has frames
 * frame_off[r] .. frame_off[r+1]) of `scores`, float32 [frames, 5] with class 4 = blank, and bases label_off[r] .. label_off[r+1])
 * of `labels`, codes 0..3.
 *
 * States.  For a read with F frames and L bases the states are s = 0..S-1, S = 2L+1.  Odd s = 2j+1 is base j; even s is blank.
 * Recurrence.  v_0(0) = x_0[blank], v_0(1) = x_0[l_0], every other v_0 is -inf;
 *     v_t(s) = best(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)) + (double)x_t[class(s)].
 * The s-2 predecessor is allowed only when s is odd and base j differs from base j-1 (the CTC repeat rule).  Values are double;
 * each step is one IEEE add of a float widened to double, so a numpy float64 restatement reproduces the result bit for bit.
 * Scores are used as given, with no log-softmax: the best path does not change when a constant is added to all five classes of
 * a frame, so normalising is the caller's business.  score_out is the sum of the given scores along the path.  Scores must be
 * finite.
 * Ties.  A later candidate replaces an earlier one only when it is strictly greater; candidates are taken in the order stay,
 * s-1, s-2; at the end state S-1 is preferred to S-2.
 * Output.  start_out[label_off[r] + j] is the first frame the path spends in state 2j+1.
 *
 * Band.  A pass of half-width w admits, at frame t, the states with |s - c(t)| <= w, c(t) = floor(t (S-1) / max(F-1, 1)) in
 * 64-bit integers; every other cell is -inf.  The first pass uses w = band0.  A pass is accepted when the end is reachable and
 * the traced path never sits on a clipped edge (s = c(t)-w > 0 or s = c(t)+w < S-1); otherwise w doubles and the read is redone,
 * inside the kernel, so a batch is one launch.  A pass with w >= S-1 is the full table and is always accepted.  band0 == 0 means
 * the full table at once, and band_out is then 0; otherwise band_out is the w of the last pass (band0 for a status-1 read).
 * max_band > 0 bounds the doubling (CHIRON_ERR_INVALID when it is below band0; ignored with band0 == 0): when the next w would
 * exceed max_band and is not yet the full table, the read ends with status 2.
 *
 * What a banded result is.  An accepted banded path is the best path INSIDE its band; it is not certified to be the global
 * optimum.  Observed on a CPU prototype of these rules: a read whose bases all occur in its first ninth and whose remaining frames
 * are noise was accepted at w = 32 with a score below the full-table optimum.  Only band0 = 0 is exact.  On squiggle-like synthetic
 * inputs (dwell geometric with mean 9, L = 40 and L = 300, band0 4, 16 and 64, final bands 16 to 64) the banded result was
 * identical to the full table.  Callers filter on the band reached and on the path's mean log-probability per frame.
 *
 * status_out: 0 aligned; 1 infeasible, F < L + the number of adjacent equal bases (F = 0 with L > 0 included); 2 band exhausted.
 * For 1 and 2 the read's start_out entries are -1 and its score_out is -inf.  L = 0 is legal: status 0, the score is the sum of the
 * blank scores, no start_out entry.
 *
 * Host arrays in, host arrays out: scores, frame_off, labels, label_off, start_out [label_off[reads]], score_out, band_out,
 * status_out [reads] are HOST memory; workspace is device memory on device_id of the size function's bytes for the same offsets,
 * band0 and max_band ("Caller's memory" above).  It holds the copied inputs and results, two recursion rows of doubles per workgroup for bands wider than
 * CHIRON_LABEL_LDS_SLOTS states, and the 2-bit back-pointer cells of every read at the widest band that read can reach.  Runs on
 * `stream` (a hipStream_t; NULL = the null stream) and synchronises it before returning.  flags: 0 (reserved).
 * CHIRON_ERR_INVALID: decreasing or negative offsets, a code above 3, a score that is not finite, band0 < 0, max_band < 0,
 * 0 < max_band < band0.  CHIRON_ERR_OVERFLOW: a read above CHIRON_LABEL_MAX_FRAMES or CHIRON_LABEL_MAX_BASES, more than 2^24
 * reads, more than 2^46 bytes of back-pointers.  All of it before anything is copied or launched.  reads == 0 is a no-op (size 0).
 * One workgroup of CHIRON_LABEL_THREADS per read; read r runs on workgroup r mod the launch's group count; every offset the
 * kernel forms is 64-bit.  The size function is host-only.                                                                       */
#define CHIRON_LABEL_MAX_FRAMES (1 << 24)
#define CHIRON_LABEL_MAX_BASES (1 << 22)
#define CHIRON_LABEL_THREADS 256
#define CHIRON_LABEL_LDS_SLOTS 4096   /* widest band (states) whose two recursion rows stay in LDS (64 KB); wider bands use workspace rows */
#define CHIRON_LABEL_MAX_GROUPS 1024  /* workgroups of one launch                                                                  */
chiron_status chiron_ctc_align_workspace_size(int64_t reads, const int64_t* frame_off, const int64_t* label_off, int32_t band0,
                                              int32_t max_band, size_t* bytes);
chiron_status chiron_ctc_align(int32_t device_id, const float* scores, const int64_t* frame_off, const uint8_t* labels,
                               const int64_t* label_off, int64_t reads, int32_t band0, int32_t max_band, uint32_t flags,
                               int32_t* start_out, double* score_out, int32_t* band_out, int32_t* status_out, void* workspace,
                               void* stream);

/* CTC log-likelihoods of many short (frame segment, candidate label) problems that point into one array of frames: what `polish`
 * asks when it rescores a pileup variant with the reads' frame posteriors.  `scores` is float32 [frames, 5], class 4 = blank, raw
 * logits, all reads concatenated.  Item i is the frame range [item_begin[i], item_end[i]) of `scores`; items may overlap and may
 * share frames.  Item i owns the candidates cand_off[i] .. cand_off[i+1]) (cand_off[0] = 0, cand_off[items] = candidates; an item
 * may own none), and candidate c is labels[label_off[c] .. label_off[c+1]), codes 0..3.  For a candidate of L bases on an item of T
 * frames x_0 .. x_{T-1}:
 *
 * Frame.  Every operand is widened to double first.  m = max_k x_k;  lp_k = (x_k - m) - log(sum_k exp(x_k - m)), the sum taken in
 * class order 0..4.
 * States.  s = 0..S-1, S = 2L+1; odd s = 2j+1 is base j (class labels[j]), even s is blank (class 4).
 * lse(v_1 .. v_n) = m + log(sum_i exp(v_i - m)) with m = max_i v_i, the sum in the order given; -inf when every v_i is -inf.
 * Recurrence.  alpha_0(0) = lp_0(4), alpha_0(1) = lp_0(labels[0]) when L >= 1, every other alpha_0 is -inf;
 *     alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2)) + lp_t(class(s)).
 * A predecessor below state 0 is -inf, and so is the s-2 predecessor unless s is odd and base j differs from base j-1: the repeat
 * rule of chiron_ctc_align.
 * Result.  loglik = lse(alpha_{T-1}(S-1), alpha_{T-1}(S-2)) (the second operand only when S >= 2): natural log, double, never
 * rounded to float.  A restatement in numpy float64 differs by the rounding of exp and log alone, a few ulp per frame.
 *
 * status_out: 0 scored; 1 infeasible, T < L + the number of adjacent equal bases (T = 0 with L > 0 included): loglik is -inf.
 * L = 0 is legal: the sum of the blank log-probabilities, 0.0 when T = 0 as well.
 *
 * Host arrays in, host arrays out: scores, item_begin, item_end [items], cand_off [items + 1], labels, label_off [candidates + 1],
 * loglik_out and status_out [candidates] are HOST memory; workspace is device memory on device_id of the size function's bytes for
 * the same frames, items, candidates and label_bytes = label_off[candidates] - label_off[0] (larger values are fine;
 * "Caller's memory" above).  It holds the
 * copied scores, the double log-softmax of EVERY frame of the call ([frames][5], computed once by score_softmax_kernel, whether an
 * item covers the frame or not), a 24-byte record per candidate, the labels and the results; `items` is checked and costs nothing.
 * Runs on `stream` (a hipStream_t; NULL = the null stream) and synchronises it before returning.  flags: 0 (reserved).
 * CHIRON_ERR_INVALID: a negative size, a negative or decreasing offset, cand_off that does not run from 0 to candidates, an item
 * outside [0, frames], a code above 3, a score that is not finite (any frame of the call).  CHIRON_ERR_OVERFLOW: an item above
 * CHIRON_SCORE_MAX_FRAMES, a candidate above CHIRON_SCORE_MAX_LABEL bases, more than 2^24 candidates or items, more than 2^40
 * frames, label_bytes above candidates * CHIRON_SCORE_MAX_LABEL.  All of it before anything is copied or launched.  items == 0 or
 * candidates == 0 is a no-op (size 0).
 * ctc_score_kernel: one wavefront per candidate, CHIRON_SCORE_THREADS / 64 to a workgroup, candidate c on wave c mod the launch's
 * waves, at most CHIRON_SCORE_MAX_GROUPS workgroups; no atomics, so a candidate's value is bitwise the same whatever else the call
 * holds and in whatever order; every offset the kernels form is 64-bit.  The size function is host-only.                        */
#define CHIRON_SCORE_MAX_FRAMES 4096   /* frames of one item                                                                      */
#define CHIRON_SCORE_MAX_LABEL 127     /* bases of one candidate: S <= 255 states, four to a lane                                 */
#define CHIRON_SCORE_THREADS 256
#define CHIRON_SCORE_MAX_GROUPS 2048   /* workgroups of one launch                                                                */
chiron_status chiron_ctc_score_workspace_size(int64_t frames, int64_t items, int64_t candidates, int64_t label_bytes, size_t* bytes);
chiron_status chiron_ctc_score(int32_t device_id, const float* scores, int64_t frames, const int64_t* item_begin,
                               const int64_t* item_end, const int64_t* cand_off, int64_t items, const uint8_t* labels,
                               const int64_t* label_off, int64_t candidates, uint32_t flags, double* loglik_out, int32_t* status_out,
                               void* workspace, void* stream);

/* Demultiplexing: which of a fixed set of short patterns (barcodes, adapters) lies in each of very many short windows (read ends),
 * how well, and where it ends.  Codes as everywhere else: 0..3, and 4 matches nothing, on either side.  A pattern p has n bases,
 * 1 <= n <= CHIRON_DEMUX_MAX_PATTERN; a window t has m bases, 0 <= m <= CHIRON_DEMUX_MAX_WINDOW.
 *
 * Per pair.  For e = 0..m let D(e) be the smallest unit-cost edit distance of p against any substring of t that ends at e (t[s:e),
 * 0 <= s <= e; the empty substring included, so D(e) <= n and D(0) = n).  The pair's result is (E, e): the smallest D, then the
 * smallest e that attains it.  It is a property of the inputs.  E equals the E of chiron_align_infix for the same pair; e need not
 * equal that call's e, which orders by matching columns before it orders by position.  Only the end is reported: a caller that needs
 * the inner boundary of a pattern at a read's tail hands the window in reversed.
 * Per window, over the call's patterns q = 0 .. patterns-1 with their group numbers pat_group[q] >= 0:
 *   best    the pattern with the smallest E, ties to the smaller q
 *   dist    that pattern's E
 *   end     that pattern's e
 *   second  the smallest E over the patterns whose pat_group differs from pat_group[best]; CHIRON_DEMUX_NONE when there is none
 * Groups let one barcode have several spellings that do not compete with each other.
 * Optional matrix.  When pair_dist_out and pair_end_out are both non-NULL, every pair's E and e are written as well, int16
 * [windows][patterns]; both NULL: not computed apart from what the window results need, not copied.  One NULL and one not is refused.
 *
 * demux_kernel (csrc/demux.hip): the bit-parallel edit-distance automaton of Myers in Hyyro's form, one pattern a lane, a pattern
 * column one 64-bit word, the first row free (horizontal input 0), exact at any distance.  With P2 the smallest power of two >=
 * min(patterns, 64), a wavefront serves 64 / P2 windows at once: lane l belongs to window slot l / P2 and takes the patterns
 * l % P2, l % P2 + P2, ... (more than one only when P2 = 64).  CHIRON_DEMUX_THREADS / 64 waves a workgroup, at most
 * CHIRON_DEMUX_MAX_GROUPS workgroups, slot groups dealt to the launch's waves round-robin.  No LDS, no atomics, every offset 64-bit;
 * a window's outputs depend on that window and the patterns alone, whatever else the call holds and in whatever order.
 *
 * Workspace (device memory), each part rounded up to 256 bytes: 40 bytes a pattern (four match masks, length, group), 16 bytes of
 * record and 16 of results a window, window_bytes + 8 windows bytes of codes (every window starts on an 8-byte boundary) and, with
 * want_matrix != 0, two int16 [windows][patterns].  Larger values of any argument are fine.  Host-only.  CHIRON_ERR_INVALID: a
 * negative argument, patterns == 0.  CHIRON_ERR_OVERFLOW: windows > 2^24, patterns > CHIRON_DEMUX_MAX_PATTERNS, window_bytes >
 * windows * CHIRON_DEMUX_MAX_WINDOW.  windows == 0 gives 0.                                                                        */
#define CHIRON_DEMUX_MAX_PATTERN 64     /* bases of one pattern: one 64-bit word a column                                          */
#define CHIRON_DEMUX_MAX_WINDOW 4096    /* bases of one window                                                                     */
#define CHIRON_DEMUX_MAX_PATTERNS 65536 /* patterns of one call: (E, q) is one 32-bit key                                          */
#define CHIRON_DEMUX_THREADS 256
#define CHIRON_DEMUX_MAX_GROUPS 2048    /* workgroups of one launch                                                                */
#define CHIRON_DEMUX_NONE 0x7FFFFFFF    /* second_out of a window whose patterns all share one group                               */
chiron_status chiron_demux_workspace_size(int64_t windows, int64_t window_bytes, int64_t patterns, int32_t want_matrix, size_t* bytes);

/* Classify `windows` windows against `patterns` patterns in one launch.  win_codes, pat_codes: HOST bytes; window w is
 * win_codes[win_off[w] .. win_off[w+1]) and pattern q is pat_codes[pat_off[q] .. pat_off[q+1]); win_off is HOST int64 [windows + 1],
 * pat_off HOST int64 [patterns + 1], both non-negative and non-decreasing; pat_group is HOST int32 [patterns].  best_out, dist_out,
 * end_out, second_out: HOST int32 [windows].  pair_dist_out, pair_end_out: HOST int16 [windows][patterns], or both NULL.  workspace:
 * device memory on device_id of chiron_demux_workspace_size(windows, win_off[windows] - win_off[0], patterns, matrix wanted) bytes ("Caller's memory" above).
 * flags: 0 (reserved).  The host packs every pattern's length and four match masks (bit i of mask c set when base i is c; a code 4
 * sets no bit), copies them and the windows in, runs on `stream` (a hipStream_t; NULL = the null stream) and synchronises it
 * before returning.  CHIRON_ERR_INVALID: unknown flags, a negative count, patterns == 0, a null array, one matrix array without the
 * other, a negative or decreasing offset, a code above 4, a pattern of 0 bases, a negative group.  CHIRON_ERR_OVERFLOW: a pattern
 * above CHIRON_DEMUX_MAX_PATTERN bases, a window above CHIRON_DEMUX_MAX_WINDOW, more than 2^24 windows, more than
 * CHIRON_DEMUX_MAX_PATTERNS patterns.  All of it before anything is copied or launched.  windows == 0 is a no-op that touches no
 * device (the counts are still checked).                                                                                           */
chiron_status chiron_demux_windows(int32_t device_id, const uint8_t* win_codes, const int64_t* win_off, int64_t windows,
                                   const uint8_t* pat_codes, const int64_t* pat_off, const int32_t* pat_group, int64_t patterns,
                                   uint32_t flags, int32_t* best_out, int32_t* dist_out, int32_t* end_out, int32_t* second_out,
                                   int16_t* pair_dist_out, int16_t* pair_end_out, void* workspace, void* stream);

/* Pileup: per genome position, what the mapped reads say there, and the consensus call.  An alignment is (pos, read, ops): pos a
 * position in concatenated genome coordinates, read the read in genome orientation (codes 0..4), ops one byte per column as
 * chiron_align_trace codes them (0 '=', 1 'X', 2 'I', 3 'D'); its '=', 'X' and 'I' columns together consume exactly the read, and m
 * is the number of its '=', 'X' and 'D' columns, the reference bases it spans.  For column j let q be the reference-consuming
 * columns before it and i the read-consuming ones.  With S = CHIRON_PILEUP_INS_SLOTS, per position g:
 *   base[g][c], c = 0..4   alignments with a '=' or 'X' column at g = pos + q whose read base read[i] is c ('=' and 'X' are not told
 *                          apart: the read base is counted, whatever the column says)
 *   del[g]                 alignments with a 'D' column at g
 *   ins[g][k][c], k < S    alignments whose (k+1)-th inserted base directly after the reference-consuming column at g is c; k is the
 *                          number of 'I' columns between that column and this one
 *   over[g]                alignments whose insertion after g is longer than S bases, each counted once (at its column k = S)
 *   depth[g]               sum_c base[g][c] + del[g]
 * An 'I' column with q = 0 (before the alignment's first reference base) or q = m (after its last) is clipping: it is counted
 * nowhere per position and goes into the call's `clipped` total.
 * The call at g, with r the reference code there, in integers only:
 *   1. depth[g] < min_depth: r is emitted, status 1 (low depth), no insertion.
 *   2. Otherwise the candidates A, C, G, T (count base[g][c]) and deletion (count del[g]) are compared by the key (count, c == r, -c)
 *      for a base and (count, 0, -9) for the deletion; the largest key wins: ties go to the reference base, then to the smaller code,
 *      and the deletion wins only when it strictly beats every base.  A winning count of 0 (only N was seen) emits r.  A winning
 *      deletion emits nothing (code 5).
 *   3. Insertion after g: slot k is emitted iff every slot below k was emitted and 2 * sum_c ins[g][k][c] > depth[g]; the base is
 *      the largest of the slot's four base counts, ties to the smaller code, and N when all four are 0.
 * over is reported and never acted on.  The counts are integer sums, so the result is a property of the inputs.
 *
 * Workspace (device memory): the per-alignment records (32 bytes each), read_bytes of codes, column_bytes of columns, the tile's
 * reference codes, CHIRON_PILEUP_PLANES int32 count planes, the depths and the 8-byte call records of tile_len positions, each part
 * rounded up to 256 bytes.  Larger values of any argument are fine.  Host-only.  CHIRON_ERR_INVALID: a negative argument.
 * CHIRON_ERR_OVERFLOW: alignments > 2^24 (which keeps every int32 count below 2^31), tile_len > CHIRON_PILEUP_MAX_TILE, read_bytes
 * or column_bytes > 2^24 * CHIRON_PILEUP_MAX_COLUMNS.                                                                             */
#define CHIRON_PILEUP_INS_SLOTS 4
#define CHIRON_PILEUP_PLANES (6 + 5 * CHIRON_PILEUP_INS_SLOTS + 1)
#define CHIRON_PILEUP_MAX_COLUMNS (1 << 24)   /* columns, and read bases, of one alignment                                        */
#define CHIRON_PILEUP_MAX_TILE (1 << 28)      /* positions of one call's tile                                                      */
#define CHIRON_PILEUP_THREADS 256             /* one workgroup per alignment; its columns are taken 256 x 4 at a time               */
chiron_status chiron_pileup_workspace_size(int64_t alignments, int64_t read_bytes, int64_t column_bytes, int64_t tile_len, size_t* bytes);

/* Count and call one genome tile [g0, g1), 0 <= g0 <= g1.  Alignment p's read is codes[read_off[p] .. read_off[p+1]), its columns
 * are ops[ops_off[p] .. ops_off[p+1]); read_off and ops_off are HOST int64 [alignments + 1], non-negative and non-decreasing; pos is
 * HOST int64 [alignments]; ref_codes is HOST uint8 [g1 - g0], the genome's codes (0..4) of the tile.  Only positions inside the tile
 * are counted; an alignment may lie partly or wholly outside it, and an insertion belongs to the tile of its anchor g.  Outputs,
 * all HOST memory: counts_out (may be NULL) int32 [CHIRON_PILEUP_PLANES][g1 - g0], PLANAR -- planes 0..4 base, 5 del, 6 + 5k + c ins,
 * the last plane over; depth_out int32 [g1 - g0]; call_out uint8 [g1 - g0][8] -- byte 0 the consensus code (0..3, 4 = N, 5 =
 * deleted), byte 1 the number of inserted bases emitted, bytes 2..5 their codes (unused ones 0), byte 6 the status (0 called, 1 low
 * depth), byte 7 zero; clipped_out int64 [1], the clipped 'I' columns of ALL alignments of the call: it does not depend on the tile
 * (a caller that tiles a genome takes it from a call that holds every alignment once, or sums it over disjoint sets).  workspace:
 * device memory on device_id of chiron_pileup_workspace_size(alignments, read bytes, column bytes, g1 - g0) bytes ("Caller's memory" above).  flags: 0
 * (reserved).  Runs on `stream` (a hipStream_t; NULL = the null stream) -- a clear of the count planes, pileup_count_kernel (one
 * workgroup of CHIRON_PILEUP_THREADS per alignment, alignment p on workgroup p mod the launch's group count, relaxed int32 atomic
 * adds; every offset 64-bit) and pileup_call_kernel (one thread per position) -- and synchronises it before returning.
 * CHIRON_ERR_INVALID for a bad offset, a code above 4 (read or reference), an op above 3, g0 < 0, g1 < g0, min_depth < 0, or an
 * alignment whose '=', 'X' and 'I' columns do not add up to its read length; CHIRON_ERR_OVERFLOW for more than 2^24 alignments, an
 * alignment past CHIRON_PILEUP_MAX_COLUMNS or a tile past CHIRON_PILEUP_MAX_TILE; all before anything is copied or launched.
 * alignments == 0 still calls the tile (all low depth, or all reference when min_depth is 0).  g1 == g0 touches no device and
 * writes clipped_out only.                                                                                                     */
chiron_status chiron_pileup(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const uint8_t* ops, const int64_t* ops_off,
                            const int64_t* pos, int64_t alignments, int64_t g0, int64_t g1, const uint8_t* ref_codes, int32_t min_depth,
                            uint32_t flags, int32_t* counts_out, int32_t* depth_out, uint8_t* call_out, int64_t* clipped_out,
                            void* workspace, void* stream);

/* Signal levels: the mean current every read spent on each of its bases, and the sums of those levels per bin -- a genome position
 * and strand, or a k-mer; what a bin means is the caller's business.  Read r has S_r = sample_off[r+1] - sample_off[r] int16 samples,
 * samples[sample_off[r] ..), and L_r = base_off[r+1] - base_off[r] bases in SIGNAL order.  Its L_r + 1 entries of `start` are
 * start[base_off[r] + r .. base_off[r+1] + r]: relative to the read's first sample, never decreasing, inside 0 .. S_r; `start` holds
 * base_off[reads] + reads entries in all.  Base n of the read owns the samples start[n] .. start[n+1]); the samples before start[0]
 * belong to nobody.  Its L_r entries of `bin` are bin[base_off[r] ..): -1, or a bin 0 .. bins - 1.
 *
 * Per base with c = start[n+1] - start[n] > 0 samples of sum s (64-bit):
 *   level = floor((2 s + c) / (2 c))      the mean rounded to nearest, halves up; floor division, not C's truncation: the samples
 *                                         [-1, -2] give -1 and [1, 2] give 2
 * It goes to level_out[base_off[r] - base_off[0] + n] whatever the bin, and when the base's bin b is not -1 the planes get
 *   events[b] += 1,  dwell[b] += c,  sum[b] += level,  sq[b] += level * level.
 * A base with c = 0 gets CHIRON_SIGNAL_EMPTY and adds nothing.  Every sum is an integer sum, so the result is a property of the
 * inputs; with at most CHIRON_SIGNAL_MAX_SAMPLES samples a call |sum| <= 2^46 and sq <= 2^61, inside int64.
 *
 * signal_kernel (csrc/signal.hip): flat over bases, a base a lane, from a 16-byte record per base that the host's checking walk
 * writes (csrc/signal_pack.h: first sample, count, bin).  Chunks of 64 consecutive bases are dealt to the launch's waves
 * round-robin, CHIRON_SIGNAL_THREADS / 64 waves a workgroup, at most CHIRON_SIGNAL_MAX_GROUPS workgroups.  A wave stages its
 * chunk's run of samples through 2 KiB of LDS, 1024 samples at a time with 16-byte loads, every sample once, and each lane sums its
 * span out of LDS.  Levels leave by plain stores, the planes get relaxed agent-scope 64-bit atomic adds.  Every offset is 64-bit.
 *
 * Workspace (device memory), each part rounded up to 256 bytes: 16 bytes of record a base, 2 bytes a sample, with want_levels != 0
 * 4 bytes a base, and CHIRON_SIGNAL_PLANES int64 planes of `bins`.  `reads` takes no room.  Larger values of any argument are fine.
 * Host-only.  CHIRON_ERR_INVALID: a negative argument.  CHIRON_ERR_OVERFLOW: samples > CHIRON_SIGNAL_MAX_SAMPLES, bases > 2^31 - 1,
 * bins > CHIRON_SIGNAL_MAX_BINS.                                                                                                   */
#define CHIRON_SIGNAL_PLANES 4            /* int64, PLANAR [4][bins]: 0 events, 1 dwell, 2 sum of levels, 3 sum of squared levels */
#define CHIRON_SIGNAL_EMPTY INT32_MIN     /* level_out of a base with no sample */
#define CHIRON_SIGNAL_MAX_SAMPLES 0x7FFFFFFF   /* samples of one call */
#define CHIRON_SIGNAL_MAX_BINS (1 << 28)
#define CHIRON_SIGNAL_THREADS 256
#define CHIRON_SIGNAL_MAX_GROUPS 2048
chiron_status chiron_signal_workspace_size(int64_t reads, int64_t samples, int64_t bases, int64_t bins, int32_t want_levels, size_t* bytes);

/* The levels and planes of `reads` reads in one launch.  samples, sample_off (int64 [reads + 1]), start, base_off (int64 [reads + 1])
 * and bin are HOST memory, the offsets non-negative and non-decreasing.  Outputs, HOST memory: planes_out int64
 * [CHIRON_SIGNAL_PLANES][bins], PLANAR (may be NULL only when bins == 0); level_out int32 [base_off[reads] - base_off[0]] (may be
 * NULL: the levels are then neither kept nor copied).  workspace: device memory on device_id of
 * chiron_signal_workspace_size(reads, the call's samples, the call's bases, bins, level_out wanted) bytes ("Caller's memory" above).
 * flags: 0 (reserved).  Copies the records and the samples in, clears the planes, runs signal_kernel on `stream` (a hipStream_t;
 * NULL = the null stream) and synchronises it before returning.  CHIRON_ERR_INVALID: unknown flags, a negative count, a null array
 * that is needed, a negative or decreasing offset, a start entry that decreases or leaves 0 .. S_r, a bin below -1 or at or above
 * bins.  CHIRON_ERR_OVERFLOW: as the size function.  All of it before anything is copied or launched.  reads == 0 (or no base at
 * all) with bins > 0 clears and returns the planes; with bins == 0 as well the call touches no device.                          */
chiron_status chiron_signal_levels(int32_t device_id, const int16_t* samples, const int64_t* sample_off, const int32_t* start,
                                   const int64_t* base_off, const int32_t* bin, int64_t reads, int64_t bins, uint32_t flags,
                                   int64_t* planes_out, int32_t* level_out, void* workspace, void* stream);

/* Signal refinement (resquiggle): move the borders between a read's bases to where the samples change level, by an exact banded
 * dynamic-time-warping DP of the samples against the level each base is expected to have (a k-mer level table's, for `squiggle
 * --refine`), seeded by borders that are roughly right (the CTC frame alignment's).
 *
 * An item is a stretch of consecutive bases of one read that all have an expected level.  Item i has S_i = sample_off[i+1] -
 * sample_off[i] int16 samples x, samples[sample_off[i] ..), L_i = base_off[i+1] - base_off[i] bases with levels e[0 .. L_i) =
 * level[base_off[i] ..), int32 inside -32767 .. 32767, and L_i + 1 initial starts a[0 .. L_i] = start_in[base_off[i] + i ..),
 * laid out as chiron_signal_levels lays out `start`: relative to the item's first sample, never decreasing, inside 0 .. S_i.
 *
 * The refined starts s[0 .. L] are the integers with
 *   s[0] = a[0] and s[L] = a[L],
 *   s strictly increasing (every base gets at least one sample),
 *   a[n] - CHIRON_REFINE_HALF <= s[n] <= a[n] + CHIRON_REFINE_HALF - 1 for 0 < n < L (64 candidates a border),
 * that minimise
 *   cost = sum over n of sum over t in s[n] .. s[n+1]) of |x[t] - e[n]|,
 * an exact integer below 2^47.  Among the minimal solutions the one with the smallest s[L-1] is taken, among those the one with
 * the smallest s[L-2], and so on down to s[1].  As a recurrence over the borders, with P the prefix sum of |x - e[n-1]|:
 *   F[0][a[0]] = 0,   F[n][s] = P(s) + min over candidates s' < s of border n-1 of (F[n-1][s'] - P(s')),   cost = F[L][a[L]],
 * and the predecessor of (n, s) is the SMALLEST s' that attains the minimum.  Where no such s exists (a[L] - a[0] < L, or bases
 * crowd more than their windows allow) cost_out is CHIRON_REFINE_INFEASIBLE and the item's start_out is a copy of its start_in.
 * An item without a base (L = 0) has cost 0 and keeps its one entry.  The samples before a[0] and from a[L] on are never read.
 * Everything is an integer, so the result is a property of the inputs.  A window wider than 64 is not offered: a second call from
 * the refined starts moves a border further.
 *
 * refine_kernel (csrc/refine.hip): a wave an item, the items dealt to the launch's waves in a loop, CHIRON_REFINE_THREADS / 64
 * waves a workgroup and at most CHIRON_REFINE_MAX_GROUPS workgroups, no workgroup barrier.  The borders are rows that run in
 * sequence; the 64 lanes are a border's candidates.  A row loads the 64 + (a[n] - a[n-1]) samples both windows span in pieces of
 * 64, scans |x - e| in int32 with an int64 carry (a piece sums below 2^23), takes a wave prefix-min of F - P in int64 and shuffles
 * it by the window shift.  The lanes that hold a strict new prefix minimum are one ballot, 8 bytes a base in the workspace; the
 * predecessor of a candidate is the highest set bit below it, and the same wave walks the rows back after its forward pass, 64
 * rows of masks per load.  Every offset is 64-bit.
 *
 * Workspace (device memory), each part rounded up to 256 bytes: the two offset arrays (8 bytes an item + 8 each), 2 bytes a
 * sample, 4 bytes a base of levels, twice 4 bytes a base and item of starts (in and out), 8 bytes a base of masks, 8 bytes an item
 * of costs.  Larger values of any argument are fine.  Host-only.  CHIRON_ERR_INVALID: a negative argument.  CHIRON_ERR_OVERFLOW:
 * items > 2^31 - 1, samples > CHIRON_SIGNAL_MAX_SAMPLES, bases > 2^31 - 1.                                                       */
#define CHIRON_REFINE_HALF 32             /* candidates of a border: a[n] - 32 .. a[n] + 31, a wave lane each */
#define CHIRON_REFINE_INFEASIBLE INT64_MAX
#define CHIRON_REFINE_THREADS 256
#define CHIRON_REFINE_MAX_GROUPS 2048
chiron_status chiron_signal_refine_workspace_size(int64_t items, int64_t samples, int64_t bases, size_t* bytes);

/* Refines `items` items in one launch.  samples, sample_off (int64 [items + 1]), level, start_in and base_off (int64 [items + 1])
 * are HOST memory, the offsets non-negative and non-decreasing.  Outputs, HOST memory: start_out int32 [base_off[items] -
 * base_off[0] + items], item i's L_i + 1 entries at base_off[i] - base_off[0] + i; cost_out int64 [items].  workspace: device
 * memory on device_id of chiron_signal_refine_workspace_size(items, the call's samples, the call's bases) bytes ("Caller's memory"
 * above).  flags: 0 (reserved).  Copies the inputs in, runs refine_kernel on `stream` (a hipStream_t; NULL = the null stream) and
 * synchronises it before returning.  CHIRON_ERR_INVALID: unknown flags, a negative count, a null array that is needed, a negative
 * or decreasing offset, a start entry that decreases or leaves 0 .. S_i, a level outside -32767 .. 32767.  CHIRON_ERR_OVERFLOW: as
 * the size function.  All of it before anything is copied or launched.  items == 0 touches no device and writes nothing; items
 * without any base touch no device either: start_out is start_in and every cost is 0.                                          */
chiron_status chiron_signal_refine(int32_t device_id, const int16_t* samples, const int64_t* sample_off, const int32_t* level,
                                   const int32_t* start_in, const int64_t* base_off, int64_t items, uint32_t flags, int32_t* start_out,
                                   int64_t* cost_out, void* workspace, void* stream);

/* Signal location: where on a reference of expected levels a stretch of raw samples comes from, without calling its bases, by an
 * exact subsequence dynamic-time-warping DP of the samples against every column of the reference (`locate`: the expected levels of
 * both strands of a genome under a k-mer level table, the first few thousand samples of a read).
 *
 * A call has one reference and `items` queries.
 *   Reference: ref_len int32 levels e[0 .. R), each inside -32767 .. 32767 or CHIRON_LOCATE_BREAK.  No path may use a break
 *     column: breaks separate contigs and strands and stand for k-mers without a level.
 *   Query i: Q_i = sample_off[i+1] - sample_off[i] int16 samples x, samples[sample_off[i] ..), 1 <= Q_i <= CHIRON_LOCATE_MAX_QUERY,
 *     which keeps every real cost below 2^30: the DP is 32-bit.
 *   Path: it assigns every sample t a column j_t with j_{t+1} in {j_t, j_t + 1}; the first and the last column are free.  A sample
 *     stays on a base or moves to the next one; every base on the path gets at least one sample (chiron_signal_refine's premise).
 *   Cost: the sum over t of |x[t] - e[j_t]|.
 *   Per end column j: D[j] is the least cost of a path that ends at j, S[j] the smallest first column among the paths that attain
 *     it.  As a recurrence over pairs ordered lexicographically (cost, then start):
 *       (D, S)[0][j] = (|x[0] - e[j]|, j),
 *       (D, S)[t][j] = lexmin((D, S)[t-1][j], (D, S)[t-1][j-1]) + (|x[t] - e[j]|, 0),
 *     and a break column, or a column with no path, holds no value.
 *   Output: for every item and every block b of CHIRON_LOCATE_BLOCK consecutive columns three int32 -- the least D[j] of the
 *     block, the smallest j that attains it, and S[j] -- or CHIRON_LOCATE_NONE in all three for a block without a path.  The
 *     blocks are part of the definition, not of the kernel: the host derives best and second-best loci from them.
 * Everything is an integer, so the result is a property of the inputs.
 *
 * locate_kernel (csrc/locate.hip): row t needs only row t-1, so the rows are cut into chunks of CHIRON_LOCATE_CHUNK and one launch
 * runs one chunk of every item; an item's DP row, (cost, start) a column, lives in the workspace between launches in two buffers
 * that are swapped each launch.  A wave takes one (item, tile of 1024 columns), the units dealt to the launch's waves in a loop,
 * CHIRON_LOCATE_THREADS / 64 waves a workgroup and at most CHIRON_LOCATE_MAX_GROUPS workgroups.  A lane keeps 16 consecutive
 * columns and their levels in registers and one column of a halo of 64 columns left of the tile; a row's sample is wave-uniform,
 * a lane's column 0 takes its left neighbour's last column by a DPP wave shift.  After r rows of a launch the halo is right from
 * its column r on, so every owned column is right after all 64; only owned columns are stored.  An item whose rows end inside a
 * launch reduces its tiles to the block triples there; no wave waits for another.  Every offset is 64-bit.
 *
 * Workspace (device memory), each part rounded up to 256 bytes: the offsets (8 bytes an item + 8), 2 bytes a sample, 4 bytes a
 * column of levels, 12 bytes an item and block of triples, and two arrays of 8 bytes an item and column of ceil(ref_len / 1024) *
 * 1024 columns (cost and start, for the two buffers).  It depends on the three counts only.  Host-only.  CHIRON_ERR_INVALID: a negative
 * argument.  CHIRON_ERR_OVERFLOW: items > 2^31 - 1, samples > CHIRON_SIGNAL_MAX_SAMPLES, ref_len > CHIRON_LOCATE_MAX_REF, more
 * than CHIRON_LOCATE_MAX_CELLS row cells (items times those columns).                                                           */
#define CHIRON_LOCATE_BREAK INT32_MIN     /* a level: no path may use this column */
#define CHIRON_LOCATE_NONE INT32_MAX      /* all three of a block's triple: no path ends in it */
#define CHIRON_LOCATE_MAX_QUERY 16384     /* samples of a query: 16384 * 65534 < 2^30 */
#define CHIRON_LOCATE_BLOCK 1024          /* columns of a block of the output */
#define CHIRON_LOCATE_MAX_REF (1 << 28)   /* columns of a reference */
#define CHIRON_LOCATE_MAX_CELLS (1ll << 40)
#define CHIRON_LOCATE_CHUNK 64            /* rows a launch */
#define CHIRON_LOCATE_THREADS 256
#define CHIRON_LOCATE_MAX_GROUPS 2048
chiron_status chiron_signal_locate_workspace_size(int64_t items, int64_t samples, int64_t ref_len, size_t* bytes);

/* Locates `items` queries on one reference.  samples, sample_off (int64 [items + 1], non-negative, increasing) and ref_level
 * (int32 [ref_len]) are HOST memory.  Output, HOST memory: block_out int32 [items][ceil(ref_len / CHIRON_LOCATE_BLOCK)][3].
 * workspace: device memory on device_id of at least the size function's bytes for (items, the call's samples, ref_len) ("Caller's
 * memory" above); workspace_bytes says how many it has.  flags: 0 (reserved).  Copies the inputs in, runs ceil(longest query /
 * CHIRON_LOCATE_CHUNK) launches of locate_kernel on `stream` (a hipStream_t; NULL = the null stream) and synchronises it before
 * returning.  CHIRON_ERR_INVALID: unknown flags, a negative count, a null array that is needed, a negative or decreasing offset,
 * an empty query, a level outside -32767 .. 32767 that is not CHIRON_LOCATE_BREAK, a workspace smaller than needed.
 * CHIRON_ERR_OVERFLOW: a query above CHIRON_LOCATE_MAX_QUERY, and as the size function.  All of it before anything is copied or
 * launched.  items == 0 touches no device and writes nothing; ref_len == 0 touches no device either and has no block to fill.    */
chiron_status chiron_signal_locate(int32_t device_id, const int16_t* samples, const int64_t* sample_off, int64_t items,
                                   const int32_t* ref_level, int64_t ref_len, int32_t* block_out, void* workspace, size_t workspace_bytes,
                                   uint32_t flags, void* stream);

/* Event detection: cuts raw samples into events of one level each, so that a location DP has one row an event and not one a
 * sample (`locate --events`).  Host-only, all in integers (csrc/event_pack.h); O(samples), no kernel and no device.
 *
 * Item i is n = sample_off[i+1] - sample_off[i] int16 samples x, 1 <= n <= CHIRON_EVENT_MAX_SAMPLES.  With a window w in 2 .. 16,
 * a radius r in 1 .. 16 and a threshold thr in 1 .. CHIRON_EVENT_MAX_THRESHOLD:
 *   For w <= i <= n - w: S1, Q1 are the sum and the sum of squares of x[i-w .. i), S2, Q2 those of x[i .. i+w), d = S1 - S2,
 *     V = (w Q1 - S1^2) + (w Q2 - S2^2), and T[i] = (w d^2 256) / max(V, 1), floor division: 256 times Welch's t^2 for two windows
 *     of equal size with population variances.  w d^2 256 <= 16 (16 * 65535)^2 256 < 2^52, so int64 holds it.
 *   T[i] = 0 for every other i of 0 .. n.
 *   i is a border iff T[i] >= thr and i is the first index of the maximum of T over [max(i-r, 0), min(i+r, n)], both ends
 *     included; 0 and n are always borders.
 *   Event k spans the samples between border k and border k+1; its level is floor((2 s + c) / (2 c)) of their sum s and count c
 *     (chiron_signal_levels' rounding: the mean, halves up).
 *   At most max_events (1 .. CHIRON_EVENT_MAX_SAMPLES) events are kept, the first ones, and truncated_out[i] says whether any
 *     was dropped: the last kept event still ends at its own border.
 * Outputs, HOST memory: count_out int32 [items]; border_out int32, item i's count_i + 1 borders (sample indices inside the item,
 * the first 0) from index sample_off[i] - sample_off[0] + i on, so the array has (samples of the call + items) entries;
 * level_out int16, item i's count_i levels from index sample_off[i] - sample_off[0] on (samples of the call entries);
 * truncated_out uint8 [items].  Entries past an item's count are left as they were.
 * CHIRON_ERR_INVALID: unknown flags (0 is the only value), a negative count, a null array that is needed, a negative or decreasing
 * offset, an empty item, w, r, thr or max_events out of range.  CHIRON_ERR_OVERFLOW: items > 2^31 - 1, an item above
 * CHIRON_EVENT_MAX_SAMPLES.  All of it before anything is written.  items == 0 writes nothing.                                    */
#define CHIRON_EVENT_MAX_SAMPLES (1 << 17)       /* samples of one item */
#define CHIRON_EVENT_MAX_WINDOW 16
#define CHIRON_EVENT_MAX_RADIUS 16
#define CHIRON_EVENT_MAX_THRESHOLD (1ll << 52)
chiron_status chiron_signal_events(const int16_t* samples, const int64_t* sample_off, int64_t items, int32_t window, int32_t radius,
                                   int64_t threshold, int32_t max_events, uint32_t flags, int32_t* count_out, int32_t* border_out,
                                   int16_t* level_out, uint8_t* truncated_out);

/* Event location: chiron_signal_locate's question for a query of event levels, whose detector may have missed a border and so left
 * a base without an event.  Everything is as in chiron_signal_locate -- reference, break columns, blocks, the triples -- except:
 *   Query i: Q_i = event_off[i+1] - event_off[i] int16 levels x, 1 <= Q_i <= CHIRON_EVENT_MAX_QUERY = 8192.
 *   Path: j_{t+1} in {j_t, j_t + 1, j_t + 2}; the move by 2 skips column j_t + 1, costs `penalty` P on top, 0 <= P <=
 *     CHIRON_EVENT_MAX_PENALTY = 65534, and is not allowed when the skipped column is a break: no path crosses a break.
 *   Recurrence:
 *       (D, S)[0][j] = (|x[0] - e[j]|, j),
 *       (D, S)[t][j] = lexmin((D, S)[t-1][j], (D, S)[t-1][j-1], (D, S)[t-1][j-2] + (P, 0) only if e[j-1] is not a break)
 *                      + (|x[t] - e[j]|, 0).
 *   A row adds at most 65535 + 65534, and 8192 * (65535 + 65534) < 2^30, which keeps every real cost below 2^30: the DP is 32-bit.
 *
 * event_locate_kernel (csrc/event_locate.hip) has locate_kernel's form: a wave per (item, tile of 1024 columns), 16 columns a lane
 * in registers, packed 64-bit (cost, start) words, CHIRON_EVENT_CHUNK = 64 rows a launch with the row in the workspace between
 * launches in two swapped buffers.  A path moves up to two columns a row, so the halo is 128 columns, two a lane: after r rows of a
 * launch it is right from its column 2 r on, and an owned column reads its last two columns of row r - 1, right for r <= 64.  A
 * lane's columns 0 and 1 take the old columns 15 and 14 of its left neighbour by two DPP wave shifts.
 *
 * Workspace: as chiron_signal_locate_workspace_size with events for samples; the same refusals.                                  */
#define CHIRON_EVENT_MAX_QUERY 8192       /* events of a query: 8192 * (65535 + 65534) < 2^30 */
#define CHIRON_EVENT_MAX_PENALTY 65534
#define CHIRON_EVENT_CHUNK 64             /* rows a launch */
#define CHIRON_EVENT_HALO 128             /* columns left of a tile that a launch recomputes: 2 a row */
chiron_status chiron_event_locate_workspace_size(int64_t items, int64_t events, int64_t ref_len, size_t* bytes);

/* Locates `items` queries of events on one reference.  events, event_off (int64 [items + 1], non-negative, increasing) and
 * ref_level (int32 [ref_len]) are HOST memory.  Output, HOST memory: block_out int32 [items][ceil(ref_len / CHIRON_LOCATE_BLOCK)][3].
 * workspace: device memory on device_id of at least the size function's bytes for (items, the call's events, ref_len) ("Caller's
 * memory" above, tests/test_gpu_event_locate.py); workspace_bytes says how many it has.  flags: 0 (reserved).  Copies the inputs in,
 * runs ceil(longest query / CHIRON_EVENT_CHUNK) launches of event_locate_kernel on `stream` (a hipStream_t; NULL = the null stream)
 * and synchronises it before returning.  CHIRON_ERR_INVALID: as chiron_signal_locate, and a penalty outside 0 ..
 * CHIRON_EVENT_MAX_PENALTY.  CHIRON_ERR_OVERFLOW: a query above CHIRON_EVENT_MAX_QUERY, and as the size function.  All of it before
 * anything is copied or launched.  items == 0 touches no device and writes nothing; ref_len == 0 touches no device either.        */
chiron_status chiron_event_locate(int32_t device_id, const int16_t* events, const int64_t* event_off, int64_t items,
                                  const int32_t* ref_level, int64_t ref_len, int32_t penalty, int32_t* block_out, void* workspace,
                                  size_t workspace_bytes, uint32_t flags, void* stream);

/* Site scoring: how well a short stretch of samples fits each of several short rows of expected levels, both ends fixed, by an
 * exact dynamic-time-warping DP (`modcall`: a read's samples around a motif site against the window's levels under a canonical
 * and under a modified k-mer level table; the difference of the two costs is the call).
 *
 * A call has `segments` sample stretches and `candidates` level rows; many candidates may share one segment, as in
 * chiron_ctc_score.
 *   Segment g: S_g = sample_off[g+1] - sample_off[g] int16 samples x, samples[sample_off[g] ..), 0 <= S_g <= CHIRON_SITE_MAX_SAMPLES.
 *   Candidate c: names a segment seg[c] in 0 .. segments - 1 and has L_c = level_off[c+1] - level_off[c] int32 levels e =
 *     level[level_off[c] ..), each inside -32767 .. 32767, 1 <= L_c <= CHIRON_SITE_MAX_COLUMNS.  Candidates come in any order, several
 *     may name one segment, a segment may have none.
 *   Path: it assigns sample t of the segment a column j_t with j_0 = 0, j_{S-1} = L - 1 and j_{t+1} in {j_t, j_t + 1}: both ends are
 *     fixed and every column gets at least one sample (chiron_signal_refine's premise).
 *   cost[c] = min over the paths of the sum over t of |x[t] - e[j_t]|, an int32: at most 4096 * 65535 < 2^29.  It is
 *     CHIRON_SITE_INFEASIBLE when there is no path: S < L, S = 0 included.
 *   As a recurrence: D[0][0] = |x[0] - e[0]|, D[0][n] has no value for n > 0, D[t][n] = min(D[t-1][n], D[t-1][n-1]) + |x[t] - e[n]|
 *     over the terms that have a value, and cost = D[S-1][L-1].
 * Everything is an integer, so the result is a property of the inputs.  No path is returned and no start column: a caller wants
 * one number a candidate.
 *
 * site_kernel (csrc/site_score.hip): a lane a candidate, the candidates dealt 64 at a time to the launch's waves in a loop,
 * CHIRON_SITE_THREADS / 64 waves a workgroup and at most CHIRON_SITE_MAX_GROUPS workgroups.  A lane keeps its 16 columns and 16
 * levels in registers, samples and levels biased by 32768 to unsigned; columns without a path hold 2^30 and need no clamp (2^30 +
 * 4096 * 65535 < 2^31).  A row updates the columns from the highest down; columns at and above L_c are computed and ignored, a
 * lane past its own S keeps its row, and column L_c - 1 is picked once at the end.  The samples go through a wave-private slice of
 * LDS in pieces of 64 a segment: every distinct segment among the wave's 64 candidates is loaded once a piece, a sample a lane,
 * into a row of its own; rows are 33 words apart, so two rows share a bank only when they are 32 rows apart, and lanes of one
 * segment read one address.  No workgroup barrier.  Every offset is 64-bit.
 *
 * Workspace (device memory), each part rounded up to 256 bytes: the segment offsets (8 bytes a segment + 8), the samples (2 bytes
 * a sample + 16, so that a 16-byte load that starts inside them ends inside them), the level offsets (8 bytes a candidate + 8), 4
 * bytes a level, 4 bytes a candidate of segment indices and 4 bytes a candidate of costs.  It depends on the four counts only.
 * Host-only.  CHIRON_ERR_INVALID: a negative argument.  CHIRON_ERR_OVERFLOW: segments > 2^31 - 1, samples >
 * CHIRON_SIGNAL_MAX_SAMPLES, candidates > 2^31 - 1, levels > 2^31 - 1.                                                          */
#define CHIRON_SITE_MAX_SAMPLES 4096      /* samples of a segment: 4096 * 65535 < 2^30 */
#define CHIRON_SITE_MAX_COLUMNS 16        /* levels of a candidate: a lane's registers */
#define CHIRON_SITE_INFEASIBLE INT32_MAX
#define CHIRON_SITE_THREADS 256
#define CHIRON_SITE_MAX_GROUPS 2048
chiron_status chiron_signal_score_workspace_size(int64_t segments, int64_t samples, int64_t candidates, int64_t levels, size_t* bytes);

/* Scores `candidates` candidates on `segments` segments in one launch.  samples, sample_off (int64 [segments + 1]), level, level_off
 * (int64 [candidates + 1]) and seg (int32 [candidates]) are HOST memory, the offsets non-negative and non-decreasing.  Output, HOST
 * memory: cost_out int32 [candidates].  workspace: device memory on device_id of at least the size function's bytes for (segments,
 * the call's samples, candidates, the call's levels) ("Caller's memory" above); workspace_bytes says how many it has.  flags: 0
 * (reserved).  Copies the inputs in, runs site_kernel on `stream` (a hipStream_t; NULL = the null stream) and synchronises it
 * before returning.  CHIRON_ERR_INVALID: unknown flags, a negative count, a null array that is needed, a negative or decreasing
 * offset, a segment above CHIRON_SITE_MAX_SAMPLES, a candidate with no level or more than CHIRON_SITE_MAX_COLUMNS, a seg entry
 * outside 0 .. segments - 1, a level outside -32767 .. 32767, a null workspace or one smaller than needed.  CHIRON_ERR_OVERFLOW: as
 * the size function.  All of it before anything is copied or launched.  candidates == 0 touches no device and writes nothing.   */
chiron_status chiron_signal_score(int32_t device_id, const int16_t* samples, const int64_t* sample_off, int64_t segments,
                                  const int32_t* level, const int64_t* level_off, const int32_t* seg, int64_t candidates,
                                  int32_t* cost_out, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

const char* chiron_last_error(void);
int32_t chiron_abi_version(void);
/* What kind of build this library is.  CHIRON_BUILD_TIMING: at least one object was compiled as a timing-only kernel variant
 * (csrc/timing_variants.h: parts of a kernel switched off to measure what they cost) -- its results are GARBAGE; the Python
 * binding refuses such a library unless CHIRON_ALLOW_TIMING_BUILD=1.  0 for the product.                               */
#define CHIRON_BUILD_TIMING 1u
uint32_t chiron_build_flags(void);

#ifdef __cplusplus
}
#endif
#endif /* CHIRON_AMD_H */
