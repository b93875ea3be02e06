/*
 * wx_align.h — C ABI of the MI355X (gfx950) forced-alignment + VAD-segmentation library
 * (libwxalign.so, built from whisperx_amd/csrc/: wx_align.hip and one file per other stage).
 *
 * The reference (NADOOIT/whisperX @ 2025-01-12) is pure Python; these entry points replace
 * the CPU functions on its alignment / VAD hot path, batched over many segments:
 *
 *   wx_trellis        <- whisperx/alignment.py:359  get_trellis(emission, tokens, blank_id)
 *   wx_backtrack      <- whisperx/alignment.py:387  backtrack(trellis, emission, tokens, blank_id)
 *   wx_merge_repeats  <- whisperx/alignment.py:438  merge_repeats(path, transcript)
 *   wx_align_dp       <- whisperx/alignment.py:242-250 (get_trellis -> backtrack ->
 *                        merge_repeats as align() chains them), fused: the trellis is never
 *                        materialised; a 1-bit decision map replaces it for the backtrack.
 *   wx_binarize       <- whisperx/vad.py:118  Binarize.__call__ (hysteresis + min-cut),
 *                        the kernel under vad.py:264 merge_chunks
 *   wx_channel_norm   <- whisperx/alignment.py:226-233 (wav2vec2 forward: feature encoder's
 *                        GroupNorm + GELU, time-major)
 *   wx_conv0_channel_norm <- the same layer with its 1-channel convolution fused (one pass
 *                        over the output)
 *   wx_attention_f32  <- whisperx/alignment.py:226-233 (wav2vec2 forward: the encoder's
 *                        self-attention, fp32)
 *   wx_vad_aggregate  <- whisperx/vad.py:198-240 VoiceActivitySegmentation.apply's
 *                        segmentation overlap-add (pyannote Inference.aggregate)
 *   wx_sincnet_stage  <- whisperx/vad.py:198-240 (the segmentation model's SincNet stages:
 *                        |.| / max-pool / instance norm / leaky ReLU, fused)
 *   wx_assign_speakers <- whisperx/diarize.py:35-67  assign_word_speakers(diarize_df,
 *                        transcript_result, fill_nearest), every segment and word of a corpus
 *   wx_log_mel        <- whisperx/audio.py:140-159  log_mel_spectrogram(audio, n_mels, padding),
 *                        every VAD chunk of a file (asr.py:141-149 preprocess) in one launch
 *   wx_whisper_stem   <- whisperx/asr.py:77-86  WhisperModel.encode (the audio encoder's two
 *                        convolutions, GELUs and positional table, fused; the layers above it
 *                        run on wx_attention_f32 and wx_add_layernorm)
 *   wx_attention_h16, wx_add_layernorm_h16 <- whisperx/asr.py:262  compute_type="float16" (the
 *                        same encoder layers on fp16 / bf16 GEMMs and attention, the residual
 *                        stream and the norms in fp32)
 *   wx_decode_attention_f32 <- whisperx/asr.py:53-62, 245-257  generate_segment_batched and
 *                        detect_language (the text decoder's self- and cross-attention of one
 *                        decode step: one query row per sequence and head)
 *   wx_decode_attention_f32_grouped, wx_beam_topk <- whisperx/asr.py:301-304  beam_size 5, the
 *                        reference's default (G beams of a chunk on the chunk's one cross-attention
 *                        K / V; the 2G best continuations of a chunk per step)
 *   wx_decode_attention_h16, wx_decode_attention_h16_grouped <- whisperx/asr.py:262
 *                        compute_type="float16" on the decoder (the two decode-step attentions
 *                        on fp16 / bf16 caches and cross-attention keys / values)
 *   wx_prefill_attention_f32, wx_prefill_attention_h16 <- whisperx/asr.py:35-45  initial_prompt /
 *                        prefix (the prompt of a batch in one forward: n queries per sequence and
 *                        head against the cache under a causal mask, and against the
 *                        cross-attention keys / values)
 *   wx_sample_token   <- whisperx/asr.py:305-312  temperatures, log_prob_threshold (the selection
 *                        of one greedy or sampled step with the token's log-probability: the
 *                        passes of the temperature fallback)
 *   wx_penalize_logits <- whisperx/asr.py:302-303  repetition_penalty, no_repeat_ngram_size (a
 *                        step's logits rewritten in place from the ids decoded so far)
 *
 * Conventions
 *   - All data pointers are DEVICE pointers (allocated by the caller; the library never
 *     allocates).  Sizes passed by value are host integers.  `stream` is a hipStream_t
 *     (NULL = default stream); every call only enqueues work on it.
 *   - Segments are CSR-packed.  Segment s has T_s = em_off[s+1]-em_off[s] emission rows
 *     starting at row em_off[s] of `em` ([sum_T, V] fp32 row-major log-probabilities) and
 *     N_s = tok_off[s+1]-tok_off[s] token ids starting at tok[tok_off[s]].
 *   - Return 0 on success or a WX_E_* / hipError_t code; wx_strerror() names it.
 *     A per-segment alignment failure (the reference's backtrack() returning None) is data
 *     (status / path_len = -1), never an error code.
 *   - Reentrant; no global mutable state; one device per call (the current device).
 *   - Semantics follow the reference's torch-CPU arithmetic bit-for-bit (fp32 adds,
 *     NaN-propagating max, strict `>` backtrack test, fp64-accumulated column-0 cumsum),
 *     except path probabilities, which use the correctly rounded fp32 exp (the reference's
 *     MKL exp differs from it by at most 1 ULP).
 */
#ifndef WX_ALIGN_H
#define WX_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    WX_OK = 0,
    WX_E_INVALID = 1001,   /* bad argument (null pointer, negative size, blank out of range) */
    WX_E_VOCAB = 1002,     /* V outside [1, WX_MAX_VOCAB] */
    WX_E_TOO_LONG = 1003,  /* a segment has more tokens than WX_MAX_TOKENS */
    WX_E_WORKSPACE = 1004, /* workspace too small (see the *_workspace_bytes queries) */
    WX_E_LAUNCH = 1005     /* kernel launch failed */
};

#define WX_MAX_VOCAB 16384   /* emission columns (V > 64: each segment's used columns are
                                gathered into a compact row of at most 256) */
#define WX_MAX_SEGMENT_COLUMNS 256 /* V > 64: distinct columns one segment may use (column 0,
                                      the blank and its token ids) */
#define WX_MAX_TOKENS 16000  /* tokens per segment (8 waves x 64 lanes x 32 cells, less halos) */

/* wx_align_dp status word: low bits = outcome, high bits = how the segment was computed */
#define WX_STATUS_MASK 15        /* 0 aligned, 1 None, 2 / 3 not computed (see wx_align_dp) */
#define WX_STATUS_RECOVERED 16   /* recomputed by the generic forward after a lost hand-off */
#define WX_STATUS_GENERIC 32     /* computed by the generic forward (> 256 distinct columns) */

const char* wx_version(void);
const char* wx_strerror(int code);

/* get_trellis (alignment.py:359-379), batched.  trellis is CSR: segment s occupies
 * (T_s+1)*(N_s+1) floats starting at element tr_off[s] (row-major [T_s+1][N_s+1]).
 * max_N = max_s N_s (host).  A segment over WX_MAX_SEGMENT_COLUMNS (V > 64) is all NaN. */
int wx_trellis(const float* em, const int64_t* em_off, int32_t V,
               const int32_t* tok, const int64_t* tok_off, const int32_t* blank_id,
               int32_t S, int64_t max_N, float* trellis, const int64_t* tr_off, void* stream);

/* Column 0 of get_trellis (alignment.py:367, `torch.cumsum(emission[:, 0], 0)`): the running
 * sums S(t) = em[0,0] + ... + em[t-1,0] for t = 0..T, accumulated in double in row order as
 * torch's CPU cumsum does, written to S[0..T] (fp64; the trellis holds them rounded to fp32).
 * em is a [T, V] fp32 row-major matrix on the device.  The fused DP's column-0 routine, one
 * wave (it exists to pin that routine bit for bit against the sequential sum). */
int wx_column0_cumsum(const float* em, int64_t T, int32_t V, double* S, void* stream);

/* backtrack (alignment.py:387-421) from a materialised trellis, batched.  The path of
 * segment s is written in forward (time-increasing) order at element em_off[s] of
 * path_tok/path_time/path_prob (capacity T_s); path_len[s] = its length or -1 (None);
 * t_start[s] = argmax of the trellis' last column (first max, NaN counted as max). */
size_t wx_backtrack_workspace_bytes(int32_t S, int64_t sum_T, int64_t max_N);
int wx_backtrack(const float* trellis, const int64_t* tr_off,
                 const float* em, const int64_t* em_off, int32_t V,
                 const int32_t* tok, const int64_t* tok_off, const int32_t* blank_id,
                 int32_t S, int64_t max_N, int64_t sum_T,
                 int32_t* path_tok, int32_t* path_time, float* path_prob,
                 int32_t* path_len, int32_t* t_start,
                 void* workspace, size_t workspace_bytes, void* stream);

/* merge_repeats (alignment.py:438-454), batched over paths stored at path_off[s] with
 * length path_len[s] (<0 = no path -> seg_count 0).  Segments are written at the same
 * offsets (capacity = path length): token index, start frame, end frame (exclusive), mean
 * probability (left-to-right fp64 sum / count, as Python's sum()). */
int wx_merge_repeats(const int32_t* path_tok, const int32_t* path_time, const float* path_prob,
                     const int64_t* path_off, const int32_t* path_len, int32_t S,
                     int32_t* seg_tok, int32_t* seg_start, int32_t* seg_end, double* seg_score,
                     int32_t* seg_count, void* stream);

/* The fused align() DP.  For every segment: trellis recurrence with a 1-bit decision map
 * (never materialised), argmax, backtrack and merge_repeats.  Outputs are CSR by tok_off:
 * seg_start/seg_end (frames, end exclusive) and seg_score of token k (the k-th
 * merge_repeats segment; a successful path always yields exactly N_s of them).
 * t_start[s] as above; status[s] & WX_STATUS_MASK = 0 aligned, 1 backtrack failed
 * (reference: None).
 * Segments the fast kernels cannot finish are recomputed in-kernel by a generic (slow,
 * barrier-per-step, ~1-3 ms per 30 s segment) forward with the same arithmetic, and say so
 * in status's flag bits: WX_STATUS_RECOVERED for a split segment whose cross-CU hand-off
 * timed out (transient starvation: another launch held the CUs), WX_STATUS_GENERIC for a
 * V > 64 segment using more than WX_MAX_SEGMENT_COLUMNS distinct emission columns.  That
 * forward keeps two rows and one decision word per cell in the kernel's LDS (3 (N + 1)
 * floats), so it holds N <= 5460 tokens in the one-wave (throughput) buckets of V > 64,
 * N <= 7167 in the latency / split buckets of V <= 64 and N <= 10921 in those of V > 64.
 * Beyond that the segment is left uncomputed and reported 2 (too many columns: split the
 * segment) or 3 (hand-off lost: re-running the call normally succeeds).
 * min_N/max_N/sum_T describe the batch (host values).
 * Split launches hand halo cells between CUs through a hand-off region of granules tagged
 * with the launch's 32-bit epoch, plus per-segment arrival counters.  wx_align_dp /
 * wx_align_dp_mode carve it out of the workspace and zero it on the stream before the launch
 * (hipMemsetAsync: the workspace may hold anything); wx_align_dp_ex takes a separate,
 * caller-owned region instead, which must be all zero before its first use and must hold
 * nothing but hand-off data afterwards: launches leave only their own granules (an older
 * launch's epoch never matches a later one) and reset the counters, so no per-launch memset
 * is needed.  One hand-off region must not be used by two launches that may run at the same
 * time (e.g. on two streams). */
size_t wx_align_dp_workspace_bytes(int32_t S, int64_t sum_T, int64_t max_N);
int wx_align_dp(const float* em, const int64_t* em_off, int32_t V,
                const int32_t* tok, const int64_t* tok_off, const int32_t* blank_id,
                int32_t S, int64_t min_N, int64_t max_N, int64_t sum_T,
                int32_t* seg_start, int32_t* seg_end, double* seg_score,
                int32_t* t_start, int32_t* status,
                void* workspace, size_t workspace_bytes, void* stream);

/* wx_align_dp with an explicit launch shape (results are identical in every mode):
 *   WX_MODE_AUTO        latency shape for batches of <= 256 segments (split over 4 CUs per
 *                       segment when the device has 4 CUs per segment), else throughput;
 *   WX_MODE_THROUGHPUT  one wave per segment up to 2048 tokens (most segments in flight);
 *   WX_MODE_LATENCY     each segment's columns spread over up to 8 waves (shortest time
 *                       per segment when the batch cannot fill the GPU), one CU each;
 *   WX_MODE_SPLIT2..4   the latency shape with each segment spread over 2..4 CUs (capped
 *                       at the device's CUs / S; 4x the emission reads).
 * wx_align_dp == wx_align_dp_mode(..., WX_MODE_AUTO) unless the environment variable
 * WX_ALIGN_MODE=0/1 forces a shape (benchmarking); WX_PARTS=2..4 opts latency launches
 * into the split. */
enum {
    WX_MODE_AUTO = -1,
    WX_MODE_THROUGHPUT = 0,
    WX_MODE_LATENCY = 1,     /* one CU per segment (WX_PARTS=2..4: split) */
    WX_MODE_LATENCY_1CU = 2, /* latency shape, one CU per segment, whatever WX_PARTS says */
    WX_MODE_SPLIT2 = 12,     /* latency shape, 2 / 3 / 4 CUs per segment */
    WX_MODE_SPLIT3 = 13,
    WX_MODE_SPLIT4 = 14
};
int wx_align_dp_mode(const float* em, const int64_t* em_off, int32_t V,
                     const int32_t* tok, const int64_t* tok_off, const int32_t* blank_id,
                     int32_t S, int64_t min_N, int64_t max_N, int64_t sum_T,
                     int32_t* seg_start, int32_t* seg_end, double* seg_score,
                     int32_t* t_start, int32_t* status,
                     void* workspace, size_t workspace_bytes, int32_t mode, void* stream);

/* Bytes of the hand-off region wx_align_dp_ex needs for a batch (0 < result; caller-owned,
 * zeroed once before first use). */
size_t wx_align_dp_handoff_bytes(int32_t S, int64_t sum_T);
/* wx_align_dp_mode with a caller-owned hand-off region (see wx_align_dp above).  handoff
 * may be NULL: then the region is carved out of the workspace and zeroed per launch. */
int wx_align_dp_ex(const float* em, const int64_t* em_off, int32_t V,
                   const int32_t* tok, const int64_t* tok_off, const int32_t* blank_id,
                   int32_t S, int64_t min_N, int64_t max_N, int64_t sum_T,
                   int32_t* seg_start, int32_t* seg_end, double* seg_score,
                   int32_t* t_start, int32_t* status,
                   void* workspace, size_t workspace_bytes,
                   void* handoff, size_t handoff_bytes, int32_t mode, void* stream);

/* Diagnostics (no device work): the kernels wx_align_dp_mode would launch for a batch of S
 * segments with token counts in [min_N, max_N] and vocabulary size V, written to buf as a
 * ';'-separated list of their rocprof names (truncated to n bytes).  Returns their number. */
int wx_align_dp_plan(int32_t S, int64_t min_N, int64_t max_N, int32_t V, int32_t mode, char* buf, size_t n);

/* Binarize.__call__ (vad.py:118-180) for n_files score columns (CSR by f_off) with
 * pyannote sliding-window geometry per file (frame i is centred at
 * 0.5*(s + (s + duration)), s = start + i*step).  onset/offset compared in fp32.
 * Regions [reg_start, reg_end] (seconds) of file f are written at reg_off[f] (capacity
 * reg_off[f+1]-reg_off[f]; F_f+1 always suffices); reg_count[f] = count, or -1 on
 * overflow.  Regions of length <= 1e-6 s are dropped (pyannote Annotation semantics). */
int wx_binarize(const float* scores, const int64_t* f_off, int32_t n_files,
                const double* sw_start, const double* sw_step, const double* sw_duration,
                float onset, float offset, double max_duration, double pad_onset, double pad_offset,
                double* reg_start, double* reg_end, const int64_t* reg_off, int64_t* reg_count,
                void* stream);

/* wx_binarize in two passes with a caller-owned workspace (same results): a chip-wide pass
 * writes per-64-frame onset/offset bit words and first-minimum records, then one wave per
 * file jumps from event to event over them (cost per event, not per frame).  total_frames =
 * f_off[n_files] (the host sizes the pre-pass grid from it). */
size_t wx_binarize_workspace_bytes(int32_t n_files, int64_t total_frames);
int wx_binarize_ex(const float* scores, const int64_t* f_off, int32_t n_files, int64_t total_frames,
                   const double* sw_start, const double* sw_step, const double* sw_duration,
                   float onset, float offset, double max_duration, double pad_onset, double pad_offset,
                   double* reg_start, double* reg_end, const int64_t* reg_off, int64_t* reg_count,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostics (no device work): the kernels wx_binarize_ex launches for these thresholds
 * (compared in fp32, as wx_binarize_ex does), ';'-separated rocprof names written to buf
 * (truncated to n bytes).  offset <= onset takes the parallel scan, offset > onset (a frame
 * may both set and reset the state, vad.py:146-175) the event-jumping state machine.
 * Returns their number. */
int wx_binarize_plan(float onset, float offset, int64_t total_frames, char* buf, size_t n);

/* Emission producer (alignment.py:226-233, the wav2vec2 forward): GroupNorm with one group
 * per channel (the first feature-encoder layer) over time-major activations x [L, C] (C % 4
 * == 0, 16-byte aligned), with the affine gamma/beta (may be NULL) and, when gelu != 0, the
 * exact erf GELU fused: y = gelu((x - mean_c) / sqrt(var_c + eps) * gamma_c + beta_c).
 * Statistics in fp64 (biased variance).  y may alias x.  Workspace: see the query. */
size_t wx_channel_norm_workspace_bytes(int32_t C);
int wx_channel_norm(const float* x, int64_t L, int32_t C, const float* gamma, const float* beta, float eps,
                    int32_t gelu, float* y, void* workspace, size_t workspace_bytes, void* stream);

/* wav2vec2's first feature-encoder layer (alignment.py:226-233, the emission forward; HF
 * Wav2Vec2GroupNormConvLayer): y[t, c] = act(GroupNorm_c(conv(x)[t, c])) with conv a 1-input-
 * channel Conv1d (K <= 16 taps, stride; w [C, K], bias [C] or NULL) over the S samples of x,
 * GroupNorm with one group per channel (statistics over time in fp64, biased variance, affine
 * gamma / beta, eps) and act the exact erf GELU when gelu != 0 (identity otherwise).  y is
 * [Lout, C] time-major, Lout = (S - K) / stride + 1.  The convolution is recomputed in the
 * second pass instead of being stored.  A per-channel constant cancels in the per-channel
 * normalisation, so bias is accepted and never read.  Equal to torch's conv + GroupNorm + GELU to
 * fp32 tolerance (its own summation order). */
size_t wx_conv0_channel_norm_workspace_bytes(int64_t L, int32_t C);
int wx_conv0_channel_norm(const float* x, int64_t S, int32_t K, int32_t stride, const float* w, const float* bias,
                          int32_t C, const float* gamma, const float* beta, float eps, int32_t gelu, float* y,
                          void* workspace, size_t workspace_bytes, void* stream);

/* wx_conv0_channel_norm with a 16-bit store (the half route of the emission producer): the same
 * passes on the fp32 waveform, expression for expression; y is [Lout, C] of `dtype` (WX_DTYPE_F16 /
 * WX_DTYPE_BF16, defined below), rounded to nearest even once on the store: bit for bit the rounding
 * of wx_conv0_channel_norm's y.  The workspace is wx_conv0_channel_norm_workspace_bytes(Lout, C).  An
 * unknown dtype is WX_E_INVALID; everything else is validated as wx_conv0_channel_norm does. */
int wx_conv0_channel_norm_h16(const float* x, int64_t S, int32_t K, int32_t stride, const float* w, const float* bias,
                              int32_t C, const float* gamma, const float* beta, float eps, int32_t gelu, int32_t dtype,
                              void* y, void* workspace, size_t workspace_bytes, void* stream);

/* wav2vec2 self-attention (alignment.py:226-233, the emission forward's encoder layers):
 * o[b, t, h, :] = softmax(scale * q[b, h, t, :] . k[b, h, :, :]^T) v[b, h, :, :], fp32, no mask,
 * head dim D = 64 only.  q/k/v are [B, H, T, 64] with element strides {batch, head, time}
 * (*_strides[0..2]; the head dim is contiguous; rows 16-byte aligned) — transformers' views
 * of the q/k/v projections need no copy; o is [B, T, H, 64] contiguous.  Every stride is a
 * multiple of 4 floats, and the time strides of k and v lie in [0, 2^23] (a key tile is addressed
 * by 32-bit byte offsets): anything else is WX_E_INVALID.  f32 MFMA, not bit-identical to torch's
 * attention (different summation order); bit-identical to wx_prefill_attention_f32 without a mask
 * on the same views (Tq = Tk = T). */
int wx_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H, int32_t T,
                     int32_t D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                     float scale, void* stream);

/* The same attention on 16-bit inputs (asr.py:262: the reference loads Whisper with
 * compute_type="float16"; the half route of WhisperEncoder): q/k/v are [B, H, T, 64] views of fp16
 * (dtype WX_DTYPE_F16) or bf16 (WX_DTYPE_BF16) elements with element strides {batch, head, time},
 * every stride a multiple of 8 and every pointer 16-byte aligned — the three slices of a fused
 * [B, T, 3 * 64 H] GEMM output are read in place; o is [B, T, H, 64] contiguous in the same type.
 * T >= 1; no workspace.  Scores are accumulated in fp32 from the 16-bit operands
 * (v_mfma_f32_32x32x16_{f16,bf16}); scale, running maximum, exponentials and running sum are fp32;
 * the unnormalised probabilities are rounded (to nearest even) to the element type as the operand
 * of the second MFMA, and the running sum is taken over those ROUNDED probabilities; O is
 * accumulated in fp32, divided by the sum in fp32 and rounded once on the store.  K / V rows at and
 * past T enter the arithmetic as zeros and no address outside the tensors is loaded from.  Row
 * (b, h, t) does not depend on B.  Validation, before anything is enqueued: B < 0, H < 1, T < 1,
 * D != 64 or an unknown dtype is WX_E_INVALID; then B == 0 is WX_OK; then a null or misaligned
 * pointer, a stride that is no multiple of 8 or more than 2^31 - 1 workgroups is WX_E_INVALID. */
#define WX_DTYPE_F16  1
#define WX_DTYPE_BF16 2
int wx_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H, int32_t T,
                     int32_t D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                     float scale, int32_t dtype, void* stream);

/* The same attention over nseg segments packed back to back in one launch (the emission
 * producer's packed encoder: every segment's rows in one [rows, H, 64] batch, each segment
 * attending only to itself — the reference's one-unpadded-forward-per-segment semantics,
 * alignment.py:217-233).  seg_rows (device, nseg + 1): segment s owns rows [seg_rows[s],
 * seg_rows[s + 1]); seg_units (device, nseg + 1): prefix of H * ceil(T_s / 32), n_units its
 * last entry.  q/k/v element strides {head, row} (*_strides[0..1]; multiples of 4 floats, the row
 * strides of k and v in [0, 2^23], as wx_attention_f32's time strides); o [rows, H, 64] contiguous.
 * split: waves per 32-query tile (1, 2 or 4; 0 = chosen from n_units).  With split 4 a segment's
 * rows are bit for bit what wx_attention_f32 returns for that segment alone. */
int wx_attention_f32_packed(const float* q, const float* k, const float* v, float* o, int32_t nseg,
                            const int32_t* seg_rows, const int32_t* seg_units, int32_t n_units, int32_t H, int32_t D,
                            const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, float scale,
                            int32_t split, void* stream);

/* wx_attention_h16 over nseg segments packed back to back in one launch (the half route of the
 * emission producer's packed encoder), with wx_attention_f32_packed's calling convention: seg_rows
 * (device int32, nseg + 1): segment s owns rows [seg_rows[s], seg_rows[s + 1]); seg_units (device
 * int32, nseg + 1): prefix of H * ceil(T_s / 64) (this kernel's unit is 64 queries), n_units its last
 * entry.  q/k/v are [1, H, rows, 64] views of fp16 / bf16 elements with element strides {head, row}
 * (*_strides[0..1], multiples of 8; pointers 16-byte aligned): the three slices of the fused
 * [rows, 3 * 64 H] q/k/v GEMM output are read in place.  o is [rows, H, 64] contiguous in the same
 * type.  Rows [seg_rows[s], seg_rows[s + 1]) of o are bit for bit what wx_attention_h16 returns for
 * that segment alone (B = 1, T = T_s, the same views offset to the segment): the same per-wave key
 * tiles and merge order.  They depend neither on nseg, nor on the other segments' contents, nor on
 * the segment's position in the pack.  A segment of T_s = 0 is legal and owns no unit.  No address
 * outside a segment's own rows is loaded for that segment; K / V rows at and past T_s enter as zeros.
 * Validation, before anything is enqueued: nseg < 0, H < 1, D != 64, an unknown dtype, n_units < 0
 * or a null q / k / v / o / stride pointer is WX_E_INVALID; then nseg == 0 or n_units == 0 is WX_OK;
 * then a null table, a misaligned pointer or a stride that is no multiple of 8 is WX_E_INVALID. */
int wx_attention_h16_packed(const void* q, const void* k, const void* v, void* o, int32_t nseg,
                            const int32_t* seg_rows, const int32_t* seg_units, int32_t n_units, int32_t H, int32_t D,
                            const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, float scale,
                            int32_t dtype, void* stream);

/* wav2vec2 positional convolution over packed segments (alignment.py:226-233: the encoder's
 * Wav2Vec2PositionalConvEmbedding, run per segment): for each segment s (rows [seg_rows[s],
 * seg_rows[s + 1]) of h [rows, D], 16-byte aligned) out[t] = GELU_erf(bias + conv(h)[t]) (+ h[t]
 * when residual), conv = Conv1d(D, D, K = 128, padding 64, groups G) with zero padding at the
 * segment's ends and the last output dropped (transformers' SamePadLayer).  D / G in {48, 64}.
 * w_packed: [G][K][Cg / 4][Cg][4], w_packed[g][j][i / 4][o][i % 4] = weight[g Cg + o][i][j].
 * seg_tiles (device, nseg + 1): prefix of ceil(T_s / 128), n_tiles its last entry.  out must not
 * alias h.  f32 MFMA: equal to torch's conv to fp32 tolerance, not bit-identical. */
int wx_posconv_packed(const float* h, int32_t D, const float* w_packed, const float* bias, int32_t G, int32_t K,
                      int32_t nseg, const int32_t* seg_rows, const int32_t* seg_tiles, int32_t n_tiles,
                      int32_t residual, float* out, void* stream);

/* wav2vec2 encoder layer's residual add + LayerNorm (alignment.py:226-233, the emission
 * forward: `layer_norm(residual + x)` twice per layer): for each of `rows` rows of D floats
 * (D in {256, 384, 512, 768, 1024, 1280}: wav2vec2's widths and Whisper's, whose pre-norm layers
 * take sum_out as the residual stream; row strides a_stride / b_stride elements, multiples of 4; all
 * pointers 16-byte aligned), s = a + b, y = (s - mean(s)) / sqrt(var(s) + eps) * gamma + beta
 * (biased variance, fp32, two passes over the row in registers).  y is [rows][D] contiguous;
 * sum_out (may be NULL) receives s in the same layout.  Equal to torch's add + LayerNorm to
 * fp32 tolerance (torch uses Welford), not bit-identical. */
int wx_add_layernorm(const float* a, const float* b, int64_t rows, int32_t D, int64_t a_stride, int64_t b_stride,
                     const float* gamma, const float* beta, float eps, float* y, float* sum_out, void* stream);

/* wx_add_layernorm between the fp32 residual stream and the 16-bit GEMMs of WhisperEncoder's half
 * route: s = a + float(b) with b [rows] x D elements of `dtype` (WX_DTYPE_F16 / WX_DTYPE_BF16; row
 * stride b_stride elements, a multiple of 8), or s = a when b is NULL (the first norm of the chain).
 * Mean, biased variance and the normalisation are wx_add_layernorm's, expression for expression, in
 * fp32; y is [rows][D] of `dtype`, rounded (to nearest even) on the store: bit for bit the rounding
 * of wx_add_layernorm(a, float(b))'s y.  sum_out (fp32, may be NULL) receives s.  Widths, alignment
 * rules (a_stride a multiple of 4; all pointers 16-byte aligned) and the validation order are
 * wx_add_layernorm's, with the dtype checked beside D. */
int wx_add_layernorm_h16(const float* a, const void* b, int64_t rows, int32_t D, int64_t a_stride, int64_t b_stride,
                         const float* gamma, const float* beta, float eps, int32_t dtype, void* y, float* sum_out,
                         void* stream);

/* wx_add_layernorm_h16 with both forms of the norm's output, for the post-norm wav2vec2 layers of
 * the emission producer's half route (norm(residual + x) is the next residual in fp32 and the next
 * GEMM operand in 16 bit): s = a + float(b), or s = a when b is NULL; y32 (fp32 [rows][D], may be
 * NULL) is bit for bit wx_add_layernorm(a, float(b))'s y, y16 ([rows][D] of `dtype`) its rounding to
 * nearest even, which is wx_add_layernorm_h16's y; sum_out (fp32, may be NULL) receives s.  One pass
 * over the row.  Widths, alignment rules and the validation order are wx_add_layernorm_h16's. */
int wx_add_layernorm_h16_dual(const float* a, const void* b, int64_t rows, int32_t D, int64_t a_stride,
                              int64_t b_stride, const float* gamma, const float* beta, float eps, int32_t dtype,
                              float* y32, void* y16, float* sum_out, void* stream);

/* VAD producer (vad.py:198-240 -> pyannote SincNet): the epilogue of one SincNet stage on the
 * time-major conv output x [B windows][L][C] (window stride x_window_stride elements, row
 * stride C; C % 4 == 0, C <= 128, 16-byte aligned): y[b][t][c] = leaky_relu(InstanceNorm1d(
 * MaxPool1d(3, 3)((|)x(|)))) with |.| when do_abs (the sinc filterbank stage), the norm's
 * biased variance over the L / 3 pooled rows, eps and affine gamma/beta (may be NULL), and
 * negative slope `slope`.  y is [B][L / 3][C] contiguous.  Statistics in fp64. */
int wx_sincnet_stage(const float* x, int64_t B, int64_t L, int32_t C, int64_t x_window_stride,
                     int32_t do_abs, const float* gamma, const float* beta, float eps, float slope,
                     float* y, void* stream);
/* wx_sincnet_stage with an input affine applied before |.|: x[b][t][c] * in_scale[b] +
 * in_shift[b][c] (both NULL or both given; in_shift 16-byte aligned), and windows that may
 * overlap (any x_window_stride >= 0, a multiple of 4).  The producer runs the sinc filterbank
 * once over the waveform and reads every window's conv output from that shared buffer
 * (window stride = hop / conv stride rows): the waveform InstanceNorm of the window, a
 * per-window affine of the input, commutes with the bias-free convolution into
 * scale * conv(x) + shift_c (shift_c = the norm's offset times filter c's tap sum). */
int wx_sincnet_stage_ex(const float* x, int64_t B, int64_t L, int32_t C, int64_t x_window_stride,
                        int32_t do_abs, const float* in_scale, const float* in_shift, const float* gamma,
                        const float* beta, float eps, float slope, float* y, void* stream);

/* VAD producer's overlap-add (vad.py:198-240 -> pyannote Inference.aggregate with the
 * multi-label max-over-classes hook): scores [n_chunks, frames_per_chunk, n_classes] fp32
 * (the segmentation model's sigmoid outputs per chunk), start_frame[c] = the file-grid frame
 * where chunk c's first frame lands (non-decreasing).  out[f] = (sum over covering chunks, in
 * chunk order, of max_k scores[c, f - start_frame[c], k]) / (number of them), NaN outputs
 * masked out; `missing` where no chunk covers f.  Feeds wx_binarize on the device. */
/* VAD producer (vad.py:198-240 -> pyannote SincNet's stage 1 on the shared-sinc route): the
 * bias-free strided filterbank convolution (K taps) of one waveform span x [n] (fp32):
 * y[t][c] = sum_{j < K} x[stride t + j] w_padded[j][c] for t < (n - K) / stride + 1, y
 * time-major [rows][C].  w_padded [KP][C]: the K taps zero-padded to KP (a multiple of 4), so
 * the kernel sums KP taps, reading zeros past the end of x.  Instantiated for pyannote's
 * C = 80, KP = 260 (K = 251), stride <= 16.  fp32 (f32 MFMA: tolerance-equal to the unfold
 * GEMM it replaces). */
int wx_sinc_filterbank(const float* x, int64_t n, int32_t stride, const float* w_padded, int32_t C, int32_t K,
                       int32_t KP, float* y, void* stream);

/* VAD producer (vad.py:198-240 -> pyannote SincNet's stages 2 and 3): Conv1d(Cin, Cout, K)
 * with no padding and stride 1 over every window of a time-major batch x [B][L][Cin]
 * (contiguous, 16-byte aligned, Cin % 4 == 0, Cin <= 80, Cout <= 64, K == 5):
 * y[b][t][o] = bias[o] + sum_{j<K, i<Cin} x[b][t + j][i] w[o][i][j], y [B][L - K + 1][Cout].
 * w_packed [K][CINP / 4][64][4] (CINP = 64 for Cin <= 64, else 80), zero-padded:
 * w_packed[j][i / 4][o][i % 4] = w[o][i][j].  fp32 (f32 MFMA: tolerance-equal to the GEMM route). */
int wx_conv1d_taps_tm(const float* x, int64_t B, int64_t L, int32_t Cin, const float* w_packed, const float* bias,
                      int32_t Cout, int32_t K, float* y, void* stream);

/* VAD producer (vad.py:198-240 -> pyannote PyanNet's LSTM): one bidirectional LSTM layer,
 * hidden size H = 128, over B sequences of T steps, both directions in one persistent launch.
 * xp [B][T][2][4H]: each step's input projection x W_ih^T + b_ih + b_hh per direction (gate
 * order i, f, g, o as torch.nn.LSTM); whh [2][4H][H]: weight_hh of the forward and reverse
 * direction; y [B][T][2H] (16-byte aligned): h of the forward direction, then the reverse.
 * h0 = c0 = 0.  fp32; equal to torch.nn.LSTM to fp32 tolerance (f32 MFMA fma chains). */
int wx_lstm_bidir_layer(const float* xp, const float* whh, float* y, int64_t B, int64_t T, int32_t H, void* stream);

int wx_vad_aggregate(const float* scores, const int64_t* start_frame, int32_t n_chunks,
                     int32_t frames_per_chunk, int32_t n_classes, int64_t n_frames, float missing,
                     float* out, void* stream);

/* assign_word_speakers (diarize.py:35-67), batched over F files in one launch: for every
 * query (qs, qe) — a segment or a timed word — the speaker whose diarization turns overlap it
 * most.  All times fp64.
 *   Turns of file f are grouped by speaker: its groups are grp_off[f] .. grp_off[f + 1] (in
 *   sorted label order, so a group's index within the file is the speaker's rank), group g
 *   owns turns turn_off[g] .. turn_off[g + 1] of turn_start / turn_end, in the table's row
 *   order (the caller stable-sorts the table by speaker rank).  G = grp_off[F] groups and
 *   n_turns = turn_off[G] turns in all (host values; turn_start / turn_end may be NULL when
 *   n_turns == 0).  Queries of file f are q_off[f] .. q_off[f + 1] of q_start / q_end,
 *   Q = q_off[F].
 *   Per query and turn x = min(end, qe) - max(start, qs) (NaN-propagating, as numpy's).  With
 *   fill_nearest == 0 the turns with x > 0 take part; otherwise every turn does, a NaN x
 *   adding nothing.  A speaker's sum runs over its participating turns in row order with Kahan
 *   compensation (y = x - c; t = s + y; c = (t - s) - y; s = t — pandas' groupby().sum()),
 *   and exists once one turn takes part.  speaker[q] = the rank of the largest sum, the
 *   lowest rank among equal sums (a NaN sum only when there is no other), or -1 when no
 *   speaker has a sum; best_sum[q] (may be NULL) = that sum, 0.0 with -1.  Non-finite times
 *   follow plain IEEE arithmetic in the recurrence.
 * Only enqueues on `stream`; no workspace.  Null pointers or negative sizes: WX_E_INVALID.
 * F == 0 or Q == 0: WX_OK without a launch.  Nothing outside speaker / best_sum [0, Q) is
 * written. */
int wx_assign_speakers(const double* turn_start, const double* turn_end, const int64_t* turn_off,
                       const int64_t* grp_off, int64_t G, int64_t n_turns,
                       const double* q_start, const double* q_end, const int64_t* q_off,
                       int32_t F, int64_t Q, int32_t fill_nearest,
                       int32_t* speaker, double* best_sum, void* stream);

/* log_mel_spectrogram (audio.py:140-159), batched over B chunks of one waveform: for chunk b,
 * what the reference returns for log_mel_spectrogram(wave[first : first + len], n_mels, pad).
 *     audio = F.pad(audio, (0, padding))                                      (audio.py:148)
 *     stft = torch.stft(audio, N_FFT, HOP_LENGTH, window=hann_window(N_FFT))  (:149-150)
 *     magnitudes = stft[..., :-1].abs() ** 2                                  (:151)
 *     mel_spec = filters @ magnitudes                                         (:153-154)
 *     log_spec = clamp(mel_spec, min=1e-10).log10()                           (:156)
 *     log_spec = maximum(log_spec, log_spec.max() - 8.0)                      (:157)
 *     log_spec = (log_spec + 4.0) / 4.0                                       (:158)
 *   The signal is the chunk followed by `pad` zeros, L = len + pad samples; torch.stft's
 *   center=True reflect extension by 200 samples on both sides is taken of that padded signal;
 *   frames 0 .. L / 160 - 1 (the last STFT frame is dropped); the maximum is the chunk's own.
 *   wave: n_wave fp32 samples on the device (4-byte alignment suffices; chunks may start
 *   anywhere).  chunk_first / chunk_len / chunk_pad: HOST arrays of B int64 (validated, and the
 *   grid is sized from them, before anything is enqueued); chunks_dev: the same 3 B values on
 *   the device, [3][B] (all firsts, all lengths, all paddings).
 *   n_mels: 80 or 128.  filters: device [n_mels][201] fp32 (the Slaney mel filterbank).
 *   basis: device, the windowed DFT basis packed as v_mfma_f32_16x16x4_f32 A fragments,
 *   [13 bin tiles][2: cos, sin][25 tap groups][64 lanes][4] fp32 (16-byte aligned): entry
 *   [bt][cs][g][lane][j] = hann(n) * (cs ? sin : cos)(2 pi k n / 400), n = 16 g + 4 (lane / 16)
 *   + j, k = 16 bt + lane % 16, hann(n) = 0.5 - 0.5 cos(2 pi n / 400); 0 for k > 200.
 *   out: chunk b, mel row m at out + (b n_mels + m) row_stride, frames 0 .. L_b / 160 - 1
 *   (L_b / 160 <= n_frames_max <= row_stride; nothing else is written; 4-byte alignment
 *   suffices).  workspace: wx_log_mel_workspace_bytes(B) bytes; after the call it holds the
 *   per-chunk maxima of the log10 values as order-preserving uint32 keys.
 * Two launches on `stream`: the fused frame gather / DFT / power / mel / log10 kernel (f32 MFMA:
 * equal to the reference to fp32 tolerance, not bit-identical), which leaves each chunk's
 * maximum in the workspace, and the floor + affine pass.  A block of 64 frames that lies wholly
 * in the zero padding skips the GEMMs (identical values; WX_NO_MEL_SKIP=1 in the environment
 * computes them).  Non-finite samples are out of scope.
 * B < 0, another n_mels, a chunk outside the waveform, L_b <= 200 (torch's reflect padding
 * refuses it too), L_b / 160 > n_frames_max, B > 65535 or a null pointer: WX_E_INVALID; a short
 * workspace: WX_E_WORKSPACE; both before anything is enqueued.  B == 0: WX_OK. */
size_t wx_log_mel_workspace_bytes(int32_t B);
int wx_log_mel(const float* wave, int64_t n_wave, const int64_t* chunk_first, const int64_t* chunk_len,
               const int64_t* chunk_pad, const int64_t* chunks_dev, int32_t B, int32_t n_mels,
               const float* filters, const float* basis, float* out, int64_t n_frames_max,
               int64_t row_stride, void* workspace, size_t workspace_bytes, void* stream);

/* The stem of Whisper's audio encoder (asr.py:77-86: WhisperModel.encode hands the features to
 * the ASR engine; the arithmetic is transformers' WhisperEncoder.forward), batched over B chunks:
 *     a1[b][t][:] = gelu(b1 + sum_{j<3} W1[:, :, j] . x[b][:, t - 1 + j])          t in [0, Tin)
 *     out[b][u][:] = gelu(b2 + sum_{j<3} W2[:, :, j] . a1[b][2u - 1 + j][:]) + pos[u][:]   u in [0, Tin / 2)
 *   with x = 0 outside [0, Tin) and a1 = 0 at row -1 of every chunk (Conv1d padding 1; the
 *   padding is the chunk's own, never a neighbouring chunk's row), gelu the exact erf form, fp32.
 *   x: chunk b, mel row m at x + b x_batch_stride + m x_row_stride (elements; x_row_stride >= Tin,
 *   4-byte alignment suffices): wx_log_mel's output, or a slice of it with fewer frames, is read
 *   in place.  n_mels: 80 or 128.  Tin even, >= 2.  D: a multiple of 64, at most 1280.
 *   w1_packed / w2_packed: conv1.weight [D][n_mels][3] / conv2.weight [D][D][3] packed as
 *   v_mfma_f32_16x16x4_f32 A fragments, [D / 16 tiles][3 taps][Cin / 16 groups][64 lanes][4] fp32
 *   (16-byte aligned): entry [ot][j][g][lane][i] = W[16 ot + lane % 16][16 g + 4 (lane / 16) + i][j].
 *   b1, b2 [D]; pos [Tin / 2][D] (embed_positions); out [B][Tin / 2][D] time-major contiguous; all
 *   16-byte aligned.  workspace: wx_whisper_stem_workspace_bytes(B, Tin, D) bytes (16-byte
 *   aligned); after the call it holds a1 [B][Tin][D] time-major, the one intermediate.
 * Two launches on `stream`, one per convolution, each an implicit GEMM over a time-major LDS
 * window (no patch buffer, no channel-major intermediate; bias, GELU and the positional row in
 * the epilogue).  Tiles are per chunk: chunk b's values are bit-identical whatever B is.  f32
 * MFMA: equal to torch's conv1d to fp32 tolerance, not bit-identical.
 * B < 0, Tin odd or < 2 (or above 2^24), another n_mels, D not a multiple of 64 or above 1280:
 * WX_E_INVALID; then B == 0: WX_OK; B > 65535, x_row_stride < Tin, a negative batch stride, a null
 * or misaligned pointer: WX_E_INVALID; a short workspace: WX_E_WORKSPACE; all before anything is
 * enqueued. */
size_t wx_whisper_stem_workspace_bytes(int32_t B, int32_t Tin, int32_t D);
int wx_whisper_stem(const float* x, int64_t x_batch_stride, int64_t x_row_stride, int32_t B, int32_t n_mels,
                    int32_t Tin, const float* w1_packed, const float* b1, const float* w2_packed, const float* b2,
                    const float* pos, int32_t D, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Attention of one decode step of Whisper's text decoder (asr.py:53-62: generate_segment_batched
 * hands the encoder output to the ASR engine; the arithmetic is transformers' WhisperDecoder.forward
 * with its key / value cache): one query row per (batch, head) against L key / value rows,
 *     o[b][h][:] = sum_{j<L} softmax_j(scale * q[b][h][:] . k[b][h][j][:]) v[b][h][j][:]
 *   fp32, no mask, head dim D == 64 only.
 *   q: row (b, h) at q + b q_strides[0] + h q_strides[1]; k / v: row (b, h, j) at
 *   k + b k_strides[0] + h k_strides[1] + j k_strides[2], v likewise (the stride arrays are HOST
 *   arrays, in elements; the head dim is contiguous; every stride a multiple of 4 and every data
 *   pointer 16-byte aligned, so that rows are).  K and V are
 *   read in place: the self-attention cache [B][H][Lcap][64] with L = the tokens so far, or the two
 *   halves of the cross-attention GEMM output [B][P][2 H 64] (row stride 2 H 64, head stride 64).
 *   Rows j >= L are never read.  o: [B][H][64] contiguous; nothing else is written.
 *   workspace: wx_decode_attention_workspace_bytes(B, H, L) bytes (16-byte aligned); after the call
 *   it holds the chunks' partial results (m, l) and acc[64].
 * The keys are cut into chunks of WX_DECODE_ATTENTION_CHUNK rows, a constant; one workgroup per
 * (chunk, head, batch) computes the chunk's softmax maximum m, sum l and weighted value sum, and a
 * second launch merges the chunks of every (batch, head) in chunk order (no launch for one chunk,
 * which the first kernel finishes itself).  No atomics, no hand-shake between workgroups.  Neither
 * the chunking nor any summation order depends on B or H: row (b, h) is bit-identical whatever the
 * batch is.  Equal to torch's scaled_dot_product_attention to fp32 tolerance, not bit-identical.
 * B < 0, H < 1, L < 1, D != 64: WX_E_INVALID; then B == 0: WX_OK; a null or misaligned pointer, a
 * stride that is no multiple of 4, B or H above 65535 (grid dimensions): WX_E_INVALID; a short
 * workspace: WX_E_WORKSPACE; all before anything is enqueued. */
#define WX_DECODE_ATTENTION_CHUNK 128
size_t wx_decode_attention_workspace_bytes(int32_t B, int32_t H, int32_t L);
int wx_decode_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H,
                            int32_t L, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                            const int64_t* v_strides, float scale, void* workspace, size_t workspace_bytes,
                            void* stream);

/* The same attention for G queries per (batch, head) that share its keys and values: the G beams
 * of one audio chunk in beam search, whose cross-attention K / V are the chunk's one [P][2 H 64]
 * block (WhisperDecoder.beam_search; the reference's default is beam_size 5, asr.py:301-304),
 *     o[b][g][h][:] = sum_{j<L} softmax_j(scale * q[b][g][h][:] . k[b][h][j][:]) v[b][h][j][:]
 *   q: row (b, g, h) at q + b q_strides[0] + g q_strides[1] + h q_strides[2]; k, v, the stride and
 *   alignment rules as above.  o: [B][G][H][64] contiguous.  1 <= G <= WX_DECODE_ATTENTION_MAX_GROUP.
 *   workspace: wx_decode_attention_grouped_workspace_bytes(B, G, H, L) bytes.
 * Same chunking, one workgroup per (chunk, head, batch): it loads every key and value row once and
 * scores it against the G queries, so K / V are read once per chunk however many beams there are;
 * the chunks are merged by the launch above's merge kernel over B G H rows.  The per-query
 * arithmetic and every summation order are those of wx_decode_attention_f32: row (b, g, h) is
 * bit-identical to what that entry point returns for the query on the same K / V, whatever B and
 * G are and whatever the other queries of the group hold.  Rows j >= L are never read.
 * B < 0, G outside 1..8, H < 1, L < 1, D != 64: WX_E_INVALID; then B == 0: WX_OK; then the checks
 * above in the same order; all before anything is enqueued. */
#define WX_DECODE_ATTENTION_MAX_GROUP 8
size_t wx_decode_attention_grouped_workspace_bytes(int32_t B, int32_t G, int32_t H, int32_t L);
int wx_decode_attention_f32_grouped(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t G,
                                    int32_t H, int32_t L, int32_t D, const int64_t* q_strides,
                                    const int64_t* k_strides, const int64_t* v_strides, float scale, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* The two entry points above on 16-bit elements (asr.py:262: compute_type="float16" covers the
 * decoder's key / value caches and the cross-attention keys and values): q, k and v hold fp16
 * (dtype WX_DTYPE_F16) or bf16 (WX_DTYPE_BF16) elements, o [B][H][64] (grouped: [B][G][H][64]) is
 * contiguous in the same type.  The layouts and the stride arrays are those above, in elements;
 * the alignment rule is wx_attention_h16's: every stride a multiple of 8 elements and every data
 * pointer 16-byte aligned.  A batch stride of 0 (K / V shared by the batch) is legal, as above.
 * Rows j >= L are never read.  The workspace is the fp32 entry points':
 * wx_decode_attention_workspace_bytes(B, H, L) / wx_decode_attention_grouped_workspace_bytes(B, G,
 * H, L) bytes, since the chunks' partial results stay fp32.
 * Arithmetic: every element is widened to fp32 exactly, the chunking, every expression and every
 * summation order are wx_decode_attention_f32's (no packed 16-bit math, no dot instruction, no
 * fused multiply-add), the division is fp32 and the quotient is rounded to nearest even once, on
 * the store.  So o is bit-identical to wx_decode_attention_f32 on the widened inputs, rounded to
 * the type; the grouped entry point has the bits of the ungrouped one for every query, and row
 * (b, h) is bit-identical whatever the batch is.
 * B < 0, H < 1, L < 1, D != 64, a dtype that is neither, G outside 1..8: WX_E_INVALID; then B == 0:
 * WX_OK; a null or misaligned pointer, a stride that is no multiple of 8, B or H above 65535 (grid
 * dimensions): WX_E_INVALID; a short workspace: WX_E_WORKSPACE; all before anything is enqueued. */
int wx_decode_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H, int32_t L,
                            int32_t D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                            float scale, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);
int wx_decode_attention_h16_grouped(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t G,
                                    int32_t H, int32_t L, int32_t D, const int64_t* q_strides,
                                    const int64_t* k_strides, const int64_t* v_strides, float scale, int32_t dtype,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* The self-attention of one decode step at a position held in DEVICE memory, with the cache append
 * fused (WhisperDecoder.start(graph=True): the launch is the same at every step, so a captured
 * graph can replay it).  With p = *pos, read by the kernels when they run:
 *   - row p of k_cache / v_cache of every (b, h) becomes the (b, h) row of k_new / v_new, bit for bit;
 *   - o[b][h][:] is the attention of q[b][h][:] over the rows 0 .. p, row p taken from k_new / v_new:
 *     bit-identical to wx_decode_attention_f32 (_h16) with L = p + 1 on the cache after that copy;
 *   - rows above p are neither read nor written;
 *   - p < 0 or p >= Lcap: nothing at all is written (defined behaviour, not an error).
 *   q, k_new, v_new: row (b, h) at x + b x_strides[0] + h x_strides[1], each with its own HOST stride
 *   array (the three column blocks of the step's [B][3 H 64] q/k/v GEMM output, read in place).
 *   k_cache, v_cache: [B][H][Lcap][64] by {batch, head, row} element strides, as k / v above.
 *   o: [B][H][64] contiguous.  pos: a device pointer to one int32, 4-byte aligned.  The alignment
 *   rules for everything else are those of wx_decode_attention_f32 (_h16: dtype and rules of
 *   wx_decode_attention_h16).  workspace: wx_decode_attention_workspace_bytes(B, H, Lcap) bytes.
 * The kernels are wx_decode_attention_f32's (one template family: the same chunks of
 * WX_DECODE_ATTENTION_CHUNK rows, per-lane arithmetic, group merge and chunk-order merge), launched
 * on a grid fixed by Lcap: (ceil(Lcap / 128), H, B) workgroups, of which those whose first row lies
 * above p return at once; the lanes that own row p take it from k_new / v_new and store it to the
 * cache, and no other workgroup touches that row.  The merge launch is enqueued whenever
 * ceil(Lcap / 128) > 1 and returns when p < 128.  The launch function neither reads *pos nor
 * allocates nor synchronises.
 * B < 0, H < 1, Lcap < 1, D != 64, (h16) a dtype that is neither: WX_E_INVALID; then B == 0: WX_OK;
 * a null or misaligned pointer (pos included), a stride that is no multiple of 4 (h16: 8), B or H
 * above 65535: WX_E_INVALID; a short workspace: WX_E_WORKSPACE; all before anything is enqueued. */
int wx_decode_self_attention_f32(const float* q, const float* k_new, const float* v_new, float* k_cache,
                                 float* v_cache, float* o, int32_t B, int32_t H, int32_t Lcap, int32_t D,
                                 const int64_t* q_strides, const int64_t* k_new_strides,
                                 const int64_t* v_new_strides, const int64_t* k_strides, const int64_t* v_strides,
                                 float scale, const int32_t* pos, void* workspace, size_t workspace_bytes,
                                 void* stream);
int wx_decode_self_attention_h16(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                 void* o, int32_t B, int32_t H, int32_t Lcap, int32_t D, const int64_t* q_strides,
                                 const int64_t* k_new_strides, const int64_t* v_new_strides,
                                 const int64_t* k_strides, const int64_t* v_strides, float scale, int32_t dtype,
                                 const int32_t* pos, void* workspace, size_t workspace_bytes, void* stream);

/* Attention of a prompt prefill (WhisperDecoder.prefill): Tq queries per (batch, head) against Tk
 * key / value rows, under a causal mask or without one,
 *     o[b][i][h][:] = sum_j softmax_j(scale * q[b][h][i][:] . k[b][h][j][:]) v[b][h][j][:]
 *         over j in [0, Tk)                        when causal < 0,
 *         over j in [0, min(Tk, causal + i + 1))   when causal >= 0 (query i sits at position causal + i).
 *   q: [B][H][Tq][64] view, row (b, h, i) at q + b q_strides[0] + h q_strides[1] + i q_strides[2]
 *      (the q slice of a fused [B][n][3 H 64] GEMM output as it is); k, v: [B][H][Tk][64] views by
 *      {batch, head, time} element strides, read in place: the self-attention cache
 *      [R][H][max_target_positions][64] (or every G-th row of it: any batch stride is legal, 0 too)
 *      and the two halves of the cross-attention [B][P][2 H 64] tensor.  The head dim is contiguous.
 *      o: [B][Tq][H][64] contiguous.  No workspace.
 *   f32: every stride a multiple of 4 floats, every pointer 16-byte aligned (wx_decode_attention_f32's
 *      rule).  h16: fp16 (WX_DTYPE_F16) or bf16 (WX_DTYPE_BF16) elements, o in the same type; every
 *      stride a multiple of 8 elements, every pointer 16-byte aligned (wx_decode_attention_h16's
 *      rule).  Both: the time strides of k and v lie in [0, 2^23] (a key tile is addressed by
 *      32-bit byte offsets).
 * One workgroup per (batch, head, 32-query tile), 4 waves over every 4th 32-key tile on
 * v_mfma_f32_32x32x2f32 with the online softmax in fp32, merged through LDS in wave order
 * (wx_attention_f32's arithmetic).  Key tiles are aligned to key 0 and a wave takes the same tiles
 * in the same order whatever the launch is; a key masked for a row contributes exactly 0 and leaves
 * the row's running maximum alone; key tiles wholly above a query tile's diagonal are skipped.  So
 * row (b, i, h) depends only on its query, on causal + i and on K / V rows 0 .. causal + i (0 ..
 * Tk - 1 without a mask): it is bit-identical whatever B, Tq and the rest of Tk are and however
 * causal + i splits into its two terms.  K / V rows at and past min(Tk, causal + Tq) are never read.
 * h16: every element is widened to fp32 exactly, every expression is the f32 kernel's (no packed
 * 16-bit math, no 16-bit MFMA) and the quotient is rounded to nearest even once, on the store: o is
 * bit-identical to wx_prefill_attention_f32 on the widened inputs, rounded to the type.
 * B < 0, H < 1, Tq < 1, Tk < 1, D != 64 or an unknown dtype: WX_E_INVALID; then B == 0: WX_OK; then a
 * null or misaligned pointer, a bad stride or more than 2^31 - 1 workgroups: WX_E_INVALID; all
 * before anything is enqueued. */
int wx_prefill_attention_f32(const float* q, const float* k, const float* v, float* o, int32_t B, int32_t H,
                             int32_t Tq, int32_t Tk, int32_t causal, int32_t D, const int64_t* q_strides,
                             const int64_t* k_strides, const int64_t* v_strides, float scale, void* stream);
int wx_prefill_attention_h16(const void* q, const void* k, const void* v, void* o, int32_t B, int32_t H, int32_t Tq,
                             int32_t Tk, int32_t causal, int32_t D, const int64_t* q_strides, const int64_t* k_strides,
                             const int64_t* v_strides, float scale, int32_t dtype, void* stream);

/* One beam-search selection step (WhisperDecoder.beam_search): B chunks of G beams, row r = b G + g
 * of logits (V fp32 columns at logits + r row_stride; nothing at columns >= V is read) and cum[r],
 * the beam's running sum of log-probabilities.
 *     lse_r = m + log(sum_t exp(x[r][t] - m)), m = max_t x[r][t], in fp32, in a summation order
 *             that depends on V alone (slices of WX_BEAM_TOPK_SLICE columns, each 4 x 1024: a
 *             lane's 16 columns in order, a butterfly over the wave, the 4 waves in order, then
 *             the slices 64 apart in order and a butterfly);
 *     candidate (g, t) of chunk b scores cum[r] + (x[r][t] - lse_r).
 * scores / index [B][2G]: the 2G best of the chunk's G V candidates, ordered by score descending,
 * then lower g, then higher logit, then lower t; index = g V + t.  (A row's candidates are
 * preselected by logit, then by lower t, before lse_r is known: within a row the score never
 * decreases with the logit.)  A logit of -inf (a suppressed id) or a cum of -inf (a dead beam) is
 * an ordinary input: such a candidate scores -inf, never NaN, and ranks after every finite one
 * in the order above; fewer than 2G finite candidates is legal.  Chunk b's output is bit-identical
 * whatever B is.  Two launches (a pass over the logits, one workgroup per slice and row; a merge,
 * one workgroup per chunk), no atomics.
 *   workspace: wx_beam_topk_workspace_bytes(B, G, V) bytes (16-byte aligned).
 * B < 0, G outside 1..8, V < 2G or V > 2^24, row_stride < V: WX_E_INVALID; then B == 0: WX_OK; a
 * null pointer, a misaligned workspace, B G above 65535 (a grid dimension): WX_E_INVALID; a
 * short workspace: WX_E_WORKSPACE; all before anything is enqueued. */
#define WX_BEAM_TOPK_SLICE 4096
size_t wx_beam_topk_workspace_bytes(int32_t B, int32_t G, int32_t V);
int wx_beam_topk(const float* logits, int64_t row_stride, const float* cum, int32_t B, int32_t G, int32_t V,
                 float* scores, int32_t* index, void* workspace, size_t workspace_bytes, void* stream);

/* One greedy or sampled selection step (WhisperDecoder.sample, the passes of decode_with_fallback):
 * R rows of V fp32 logits at logits + r row_stride (read, never written; nothing at columns >= V is
 * read; no alignment is asked of row_stride).  For row r, with step = *step read on the device (so a
 * captured launch draws a new stream at every replay):
 *     m_t = -inf where suppress[t] != 0 (suppress may be NULL: no mask), else the logit; a logit of
 *           -inf is an ordinary input.
 *     done[r] != 0 on entry: token[r] = eot, logprob[r] = 0, sum_logprob[r] and done[r] left alone.
 *     every m_t = -inf: token[r] = eot, logprob[r] = 0, done[r] = 1, sum_logprob[r] left alone.
 *     otherwise token[r] = argmax_t z_t, the lowest t on ties, with
 *         temperature == 0:  z_t = m_t;
 *         temperature > 0:   z_t = m_t / temperature + g_t (Gumbel-max: a draw from
 *                            softmax(m / temperature)), g_t = -log(-log(u_t)),
 *                            u_t = ((x_t >> 9) + 0.5) 2^-23 (exact in fp32, never 0 or 1),
 *                            x_t = word (t & 3) of Philox4x32-10 with counter
 *                            (t >> 2, r, low word of step, high word of step) and key
 *                            (low word of seed, high word of seed);
 *       all in fp32 (a correctly rounded division, logf, one addition);
 *     logprob[r] = m_token - lse, lse = M + log(sum_t exp(m_t - M)), M = max_t m_t: the
 *       log-probability at temperature 1 whatever the temperature is, in fp32, in a summation order
 *       that depends on V alone (slices of WX_SAMPLE_TOKEN_SLICE columns, each 4 x 1024; in a wave
 *       lane i holds columns 256 e + 4 i + j of its 1024, e and j in 0..3: a lane's 16 columns in
 *       ascending order, a butterfly over the wave, the 4 waves in order, then the slices 64 apart in
 *       order and a butterfly);
 *     sum_logprob[r] += logprob[r] (one fp32 addition; sum_logprob may be NULL);
 *     done[r] |= (token[r] == eot).
 * Row r's outputs are bit-identical whatever R is and whatever the other rows hold.  Two launches (a
 * pass over the logits, one workgroup per slice and row; a merge, one wave per row), no atomics.
 *   workspace: wx_sample_token_workspace_bytes(R, V) bytes (16-byte aligned).
 * R < 0, V < 1 or V > 2^24, row_stride < V, a negative or non-finite temperature, eot outside
 * [0, V): WX_E_INVALID; then R == 0: WX_OK; a null pointer (suppress and sum_logprob excepted), a
 * misaligned workspace, R above 65535 (a grid dimension): WX_E_INVALID; a short workspace:
 * WX_E_WORKSPACE; all before anything is enqueued. */
#define WX_SAMPLE_TOKEN_SLICE 4096
size_t wx_sample_token_workspace_bytes(int32_t R, int32_t V);
int wx_sample_token(const float* logits, int64_t row_stride, int32_t R, int32_t V, const uint8_t* suppress,
                    float temperature, uint64_t seed, const int64_t* step, int64_t eot, uint8_t* done,
                    int64_t* token, float* logprob, float* sum_logprob, void* workspace, size_t workspace_bytes,
                    void* stream);

/* The repetition penalty and the no-repeat n-gram ban of one decoding step (WhisperDecoder's
 * repetition_penalty and no_repeat_ngram_size), applied in place to R rows of V fp32 logits at
 * logits + r row_stride ahead of the selection.  Row r's history is
 *     h_i = history[i step_stride + r hist_row_stride], i in [0, L),
 *     L = min(max(*count + count_offset, 0), max_history),
 * with *count read on the device (so a captured launch sees a longer history at every replay) and
 * the sum taken in 64 bits.  Both layouts are the strides' choice: step-major [L][R] is
 * (R, 1), row-major [R][cap] is (1, cap).  An id outside [0, V) is skipped: it matches nothing and
 * writes nothing (ids are compared as 64-bit values; they are narrowed only after the range check).
 *   repetition penalty rho = repetition_penalty:
 *     for every distinct in-range id t of the history, once however often it occurs:
 *         x = logits[r][t];  logits[r][t] = x < 0 ? x rho : x / rho
 *     in fp32: one multiplication or one correctly rounded division.  -inf stays -inf, -0 stays -0
 *     (it is not below 0: it is divided).  rho == 1 writes nothing.
 *   no-repeat n-gram, n = no_repeat_ngram_size:
 *     n == 0: nothing.  n >= 1: for every j in [0, L - n] (none when L < n) with
 *         h[j .. j + n - 2] == h[L - n + 1 .. L - 1]
 *     logits[r][h[j + n - 1]] = -inf.  For n == 1 the comparison is empty, so every history id is
 *     banned.  Matches that overlap the suffix count.  A skipped id inside either window makes the
 *     window match nothing, and a skipped h[j + n - 1] bans nothing.
 *   A ban wins over the penalty on the same column: the column is -inf.
 * Columns that neither rule names, columns >= V and everything outside the R rows are never written
 * (nor read).  A named column is stored once.  Row r's result is bit-identical whatever R is and
 * whatever the other rows hold.  One launch, one workgroup per row; no workspace, no atomics.
 * R < 0, V < 1 or V > 2^24, row_stride < V, a repetition_penalty that is not finite or not above 0,
 * n < 0, max_history outside [0, WX_PENALTY_MAX_HISTORY]: WX_E_INVALID; then R == 0 or
 * max_history == 0: WX_OK; then a null pointer or R above 65535 (a grid dimension): WX_E_INVALID;
 * all before anything is enqueued.  The strides are the caller's: every h_i above must lie in
 * history's allocation. */
#define WX_PENALTY_MAX_HISTORY 1024
int wx_penalize_logits(float* logits, int64_t row_stride, int32_t R, int32_t V, const int64_t* history,
                       int64_t step_stride, int64_t hist_row_stride, const int64_t* count, int32_t count_offset,
                       int32_t max_history, float repetition_penalty, int32_t no_repeat_ngram_size, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WX_ALIGN_H */
