/*
 * ds2hip.h -- C ABI of libds2hip.so: the MI355X (gfx950) DeepSpeech2 hot path.
 *
 * The reference (igormq/aes-lac-2018) has no FFI of its own: its hot path bottoms out in
 * torch.nn modules (cuDNN/ATen), librosa and the warp-ctc binding.  Each entry point below
 * replaces one of those call sites; the citation gives the reference line it stands in for.
 * Bindings: aes-lac-2018_amd/ds2hip/lib.py (ctypes); INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - all tensors are dense fp32 row-major unless stated, int32 for lengths/labels;
 *   - the caller owns every buffer (inputs, outputs, saved-for-backward tensors, workspaces);
 *     the library never allocates or frees device memory and keeps no mutable global state;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls only enqueue work;
 *   - return value 0 = ok, negative = error (DS2_ERR_*); ds2_last_error() returns a
 *     thread-local message.  No exceptions cross the boundary.
 *
 * Shapes: B batch, T_in spectrogram frames, F=161 bins, T1 = (T_in+9)/2+1 frames after conv1,
 * T = T1-10 frames after conv2, H GRU hidden size, A alphabet size (blank = 0).
 */
#ifndef DS2HIP_H
#define DS2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS2_OK 0
#define DS2_ERR_ARG (-1)
#define DS2_ERR_LAUNCH (-2)
#define DS2_ERR_UNSUPPORTED (-3)

const char* ds2_last_error(void);
/* The ABI revision this header describes.  ds2_version() of the loaded library must return exactly this number: signatures
 * have changed between revisions without a change of symbol name (round 3: an amplitude-scale argument in
 * ds2_pcm16_to_float / ds2_gain_requantize; round 4: ds2_conv2_dgrad takes the size of its workspace), so a binding built
 * against another revision mis-passes arguments.  ds2hip/lib.py refuses to load a library whose number differs. */
#define DS2_ABI_VERSION 404
int ds2_version(void);
/* A digest of the sources the loaded binary was built from (csrc/build.py: source_id(); "unstamped" for a build made without
 * build.py).  The Python binding recomputes it from the tree beside it and refuses a binary built from other sources, so a
 * stale .so cannot be tested or benchmarked by accident (DS2_SKIP_BUILD_CHECK=1 overrides, for binary-only installs). */
const char* ds2_build_id(void);

/* ------------------------------------------------------------------ frontend
 * Replaces ToSpectrogram.__call__ (librosa branch), codes/transforms.py:94-119, run per
 * utterance in codes/data.py:61-62, and the zero-padding collate of codes/data.py:132-152.
 *   wav          concatenated clips, clip b = wav[wav_offsets[b] .. wav_offsets[b+1])
 *   wav_offsets  (B+1) int64 device
 *   out          (B, t_max, 161), zero-filled past each clip's 1 + L_b/160 frames
 *   stats_ws     workspace, >= ds2_spectrogram_ws_bytes(B, t_max) bytes
 * STFT: reflect-pad 160, frame 320 / hop 160, symmetric Hann, |rFFT|, log1p, then per-clip
 * (S - mean) / (std_unbiased + eps).
 */
size_t ds2_spectrogram_ws_bytes(int B, int t_max);
int ds2_spectrogram_fwd(const float* wav, const int64_t* wav_offsets, int B, int t_max, int normalize,
                        float eps, float* out, void* stats_ws, void* stream);

/* ------------------------------------------------------------------ waveform decode + augmentation
 * Replace the per-clip host work of ToTensor (codes/transforms.py:130-224): torchaudio.load of a 16-bit PCM
 * file, and -- for training clips with augment=True -- `sox ... -b 16 -e si <out> tempo T gain G` through a
 * temporary file (:185-218).  The loader ships int16 samples; these run after collate on the whole minibatch.
 *   ds2_pcm16_to_float   out[i] = pcm[i] * scale                                  (n samples, any concatenation).  The
 *                        amplitude scale is torchaudio.load's contract (codes/transforms.py:156-161), which changed between
 *                        torchaudio versions: 1/32768 gives [-1, 1); 65536 gives the un-normalised int32-range floats of
 *                        the mid-2018 master (a 16-bit sample read by sox as a 32-bit one).  log1p is not scale invariant.
 *   ds2_wsola_tempo      time-scale change without pitch change (WSOLA, sox's default 82 / 14.68 / 12 ms segment /
 *                        search / overlap -> seg, half = search/2, ovl in samples).  Clip b = x[in_offsets[b] ..
 *                        in_offsets[b+1]) -> out[out_offsets[b] .. out_offsets[b+1]).  The segment schedule is data
 *                        independent: bases[base_offsets[b] + k] is the rounded ideal input position of segment k
 *                        (running sum of tempo * (seg - ovl)); zero segments = copy.  The output length follows from
 *                        the schedule: (nseg + 1) * (seg - ovl) + ovl.  Correlations in float64, first maximum wins.
 *                        The algorithm is specified in oracle/audio.py (sox's own implementation is not in the
 *                        reference tree: parity with sox is not claimed).
 *   ds2_gain_requantize  y = x * gain[b]; out = clip(rint(y * 32768), -32768, 32767) * out_scale   (x in [-1, 1); the gain
 *                        in linear units, 10^(dB/20); rounding half to even; out_scale as ds2_pcm16_to_float's scale),
 *                        in place allowed
 */
int ds2_pcm16_to_float(const int16_t* pcm, size_t n, float scale, float* out, void* stream);
int ds2_wsola_tempo(const float* x, const int64_t* in_offsets, const int64_t* out_offsets, const int32_t* bases,
                    const int32_t* base_offsets, int B, int seg, int ovl, int half, float* out, void* stream);
int ds2_gain_requantize(const float* x, const int64_t* offsets, const float* gain, int B, float out_scale, float* out,
                        void* stream);

/* ------------------------------------------------------------------ noise injection
 * Stands where NoiseInjection.__call__ would run (codes/transforms.py:254-287), between the waveform loader and the
 * spectrogram: additive background noise at a drawn level relative to the clip's rms.  The reference's class raises on its
 * first call (`noise.size` is a method, :268-269), so this is its evident intent; one launch pair mixes the whole minibatch.
 *   wav, offsets   clip b = wav[offsets[b] .. offsets[b+1]), n_b samples: the float output of the decode above
 *   bank           the int16 samples of every noise recording, concatenated; clip b's recording is
 *                  bank[noise_lo[b] .. noise_lo[b] + noise_len[b]).  noise_len[b] == 0: no noise drawn for this clip --
 *                  out equals wav bit for bit there and coef[b] = 0
 *   noise_start    first sample of the crop, in [0, noise_len[b]) (clamped into it; nothing outside the recording is read)
 *   level          (B) float, the drawn noise level
 * For i in [0, n_b):  nz[i] = (float)bank[noise_lo + (noise_start + i) mod noise_len] * noise_scale (one rounded multiply, as
 * ds2_pcm16_to_float; a recording shorter than the clip repeats);  Ex = sum wav[i]^2, En = sum nz[i]^2 in float64 over exact
 * products;  coef = (float)(level * sqrt(Ex / n) / sqrt(En / n)) -- the reference's noise_level * signal_energy /
 * noise_energy with rms energies -- and 0 when En == 0 (a silent crop) or the quotient is not finite;
 * out[i] = wav[i] + coef * nz[i], the product and the sum each rounded once (no fma).  coef == 0 copies wav (bit for bit).
 * out == wav (in place) is allowed.  coef (B floats) may be NULL.
 * Two kernels: per-chunk (Ex, En) partials into ws (DS2_NOISE_CHUNK samples per workgroup, chunks counted from the clip's own
 * start), then every workgroup sums its clip's partials in index order and mixes its chunk.  No atomics: a clip's output
 * bits do not depend on its position in the batch, on the other clips, on its offset in wav, or on what ws held.
 * ws >= ds2_noise_mix_ws_bytes(B, longest clip) bytes, need not be zeroed; ws_bytes fixes the grid (ws_bytes / (16 B) chunks
 * per clip; the workgroups of a longer clip take several chunks each, so every sample is still mixed) and must hold at
 * least one partial per clip.  B in 1..65535; noise_scale > 0 (the frontend's amplitude scale: the ratio of the energies
 * cancels it, but the noise goes through the same conversion as the speech).
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_NOISE_CHUNK 4096
size_t ds2_noise_mix_ws_bytes(int B, size_t max_clip_len);
int ds2_noise_mix(const float* wav, const int64_t* offsets, int B, const int16_t* bank, const int64_t* noise_lo,
                  const int64_t* noise_len, const int64_t* noise_start, const float* level, float noise_scale, float* out,
                  float* coef, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ reverberation
 * Convolution of every drawn clip of a minibatch with a room impulse response (RIR), between the gain stage and the noise
 * stage above (tempo -> gain -> reverberation -> noise -> spectrogram -> SpecAugment).  The reference has no such stage:
 * nothing here is parity, every rule is a decision.
 *   wav, offsets   clip b = wav[offsets[b] .. offsets[b+1]), n_b samples: the float output of the decode above
 *   bank           the float taps of every RIR, concatenated; clip b's RIR is h = bank[rir_lo[b] .. rir_lo[b] + rir_len[b]),
 *                  K = rir_len[b] taps, at most DS2_REVERB_MAX_TAPS (clamped into [0, that]).  The bank rule (host,
 *                  codes/transforms.py Reverb): per 16-bit mono 16 kHz file, in float64, s = int16 / 32768, p = the first
 *                  index of max |s|, h = s[p : p + max_taps] / s[p], trailing zeros stripped, rounded to float32 -- so
 *                  h[0] == 1 exactly, the direct path is not delayed and what precedes the peak is dropped.
 *   rir_len[b]==0  no draw: out equals wav bit for bit there (-0.0 and NaN payloads included) and gain[b] = 1
 * Convolution:  y[n] = sum_{k=0}^{min(n, K-1)} h[k] x[n-k]  for n in [0, n_b), in fp32: the clip keeps its length, the tail
 * is cut, and the history before the clip's first sample is zero -- never the neighbouring clip.  Each y[n] is one chain of
 * fused multiply-adds in ONE accumulator, from the last tap down to h[0] (v_mfma_f32_16x16x4_f32, exact fp32; zero products
 * stand in the chain where the 16x16 tile reaches past the RIR).  Nothing outside the clip or outside the RIR is loaded, so
 * a NaN next door never reaches a product; a NaN or infinity INSIDE the clip or its RIR may spread to outputs up to 31
 * samples away from those the sum itself names (0 * NaN in those zero products).
 * Level (keep_level = 1):  Ex = sum x[n]^2 and Ey = sum y[n]^2 in float64 over exact products, over x and over the kernel's
 * own fp32 y, in a fixed order;  gain = (float)sqrt(Ex / Ey), and 1 when Ey == 0 or the quotient is not finite;
 * out[n] = gain * y[n], ONE rounded fp32 multiply.  keep_level = 0: out = y, gain = 1.  Floats out, not requantised.
 * out == wav is refused (every output reads K inputs); samples of out outside every clip are not written.  gain (B floats)
 * may be NULL.  Two kernels: a workgroup convolves DS2_REVERB_TILE consecutive outputs of one clip (tiles counted from the
 * clip's own start), staging taps and samples through LDS in passes of DS2_REVERB_TAPS_STEP taps, writes the unscaled y to
 * out and ONE (Ex, Ey) pair to ws; then every workgroup sums its clip's pairs in index order and scales its tile in place.
 * No atomics: a clip's output bits and its gain depend on the clip and its RIR only -- not on its position in the batch or
 * in memory, the other clips, what ws held, or a ws larger than required.
 * ws >= ds2_reverb_ws_bytes(B, longest clip) bytes, need not be zeroed; ws_bytes fixes the grid (ws_bytes / (16 B) tiles per
 * clip; with less than required the workgroups of a longer clip take several tiles each, every sample is still produced,
 * and the order of the energy sum follows the grid) and must hold at least one pair per clip.  B in 1..65535.
 * DS2_REVERB_FORM=valu in the environment selects the plain vector-ALU form of the same sum (the timing baseline).
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_REVERB_TILE 2048
#define DS2_REVERB_TAPS_STEP 512
#define DS2_REVERB_MAX_TAPS 65536
size_t ds2_reverb_ws_bytes(int B, size_t max_clip_len);
int ds2_reverb(const float* wav, const int64_t* offsets, int B, const float* bank, const int64_t* rir_lo,
               const int64_t* rir_len, int keep_level, float* out, float* gain, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ sample-rate conversion (csrc/resample.hip)
 * 16-bit PCM of any rate and 1..8 channels to mono at another rate, before everything above: the reference handed its files
 * to sox, which is not part of this project.  Nothing here is parity with sox: the filter (host, ds2hip/ops.py
 * resample_design: a Kaiser-windowed sinc, 24 zero crossings, roll-off 0.95, beta 9) and every rule below are decisions,
 * and nobody has measured their effect on WER.
 *   pcm, in_offsets   clip b = pcm[in_offsets[b] .. in_offsets[b+1]) holds n_b = (in_offsets[b+1] - in_offsets[b]) / channels
 *                     interleaved frames; (B+1) int64 on the device.  A length that is not a multiple of `channels` (or a
 *                     negative one) is DS2_ERR_ARG and nothing is written
 *   taps              (L, K) float32, K odd, h = (K - 1) / 2: row p is the filter at the fractional position p / L
 * Downmix:  s[j] = sum_c pcm[in_offsets[b] + j * channels + c], an exact integer (|s| <= 2^18), exact as a float.
 * Polyphase FIR:  for output m in [0, ds2_resample_out_len(n_b, L, M)):  t = m * M (int64: an hour at M = 441 passes 2^31),
 * i0 = t / L, p = t % L,  y = sum_{k=0}^{K-1} taps[p * K + k] * s[i0 + k - h],  where s outside [0, n_b) is zero -- never the
 * neighbouring clip of the flat buffer, and nothing outside the clip is loaded.  The sum is ONE chain of fused multiply-adds
 * in one fp32 accumulator that starts at +0 and takes k = 0, 1, .. K - 1 in that order, the zero products of the padding
 * included (they change no bit while the taps are finite); the order does not depend on the grid, the tile or the batch.
 * Output:  v = y * (1.0f / channels), one rounded multiply, skipped for one channel;
 * out[out_offsets[b] + m] = (int16) clamp(rint(v), -32768, 32767), rounding half to even.  Elements of out outside every
 * clip are not written; out must not overlap pcm.
 * One kernel, no atomics, no workspace: a workgroup produces DS2_RESAMPLE_TILE consecutive outputs of one clip (tiles counted
 * from the clip's own start) and stages the downmixed span of the tile through LDS.  A clip's output bits depend on the clip
 * and the taps only -- not on B, on its position in the batch or in memory, or on the other clips.
 * L = M = K = 1, taps = [1], channels = 1 copies the input bit for bit.
 * Limits (DS2_ERR_ARG outside them): B in 1..65535, channels in 1..8, L in 1..1024, M in 1..4096, K odd in 1..1023.
 * Unlike the other entry points this one WAITS on `stream` once before its launch: it reads the B + 1 input offsets back, to
 * check the lengths before anything is written and to size the grid by the longest clip.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_RESAMPLE_TILE 1024
size_t ds2_resample_out_len(size_t n_frames, int L, int M);      /* (n_frames * L + M - 1) / M */
int ds2_resample(const int16_t* pcm, const int64_t* in_offsets, int B, int channels, int L, int M, const float* taps, int K,
                 int16_t* out, const int64_t* out_offsets, void* stream);

/* ------------------------------------------------------------------ speed perturbation / per-clip ratio (csrc/resample_var.hip)
 * Resampling a training clip by 0.9 / 1.0 / 1.1 so that duration and pitch move together (Ko et al. 2015), in front of the
 * tempo stage (speed -> tempo -> gain -> reverberation -> noise -> spectrogram -> SpecAugment).  The reference has no such
 * stage: the factors, the filter (ds2hip/ops.py speed_design: resample_design at 16000 * factor Hz) and every rule below are
 * decisions, and nobody has measured their effect on WER.  ONE launch for a minibatch in which every clip has its own ratio
 * and filter table, and -- unlike ds2_resample -- NO wait on `stream`: nothing is read back.
 *   pcm, in_offsets   clip b = pcm[in_offsets[b] .. in_offsets[b+1]), n_b mono int16 samples; (B+1) int64 on the device
 *   out, out_offsets  clip b's outputs go to out[out_offsets[b] ..); (B+1) int64 on the device (the caller computes them
 *                     with ds2_resample_out_len; the last entry is not read)
 *   table_ids         (B) int32 on the device: the table of clip b
 *   tables_host       n_tables entries {L, M, K, tap_offset} in HOST memory, 1..DS2_RESAMPLE_VAR_TABLES of them: validated
 *                     before the launch and handed to the kernel by value (the array may be reused when the call returns).
 *                     Table i is the (L, K) float32 table tap_bank[tap_offset .. tap_offset + L * K), laid out as
 *                     ds2_resample's taps; bank_floats is the size of tap_bank in floats (device)
 *   max_out           the longest clip's output count, which the caller knows: it sizes the grid
 * Arithmetic: clip b with table (L, M, K, taps) gets exactly ds2_resample's polyphase rule at channels = 1 --
 * n_out = ds2_resample_out_len(n_b, L, M), t = m * M in int64, i0 = t / L, p = t % L, ONE chain of fused multiply-adds in one
 * fp32 accumulator from +0 over k = 0 .. K - 1 upwards, samples outside the clip zero by a predicate on the index (nothing
 * outside the clip is loaded), out = (int16) clamp(rint(y), -32768, 32767), halves to even.  A clip's output bits EQUAL those
 * of ds2_resample launched on that clip alone with the same (L, M, taps, K); they depend on nothing else -- not on B, the
 * clip's position in the batch or in memory, the other clips or their tables, or a max_out larger than needed.
 * L = M = K = 1, taps = [1] copies the clip bit for bit.  Elements of out outside every clip are not written; out must not
 * overlap pcm.
 * One kernel, no atomics, no workspace: a workgroup produces DS2_RESAMPLE_TILE consecutive outputs of one clip, as
 * ds2_resample's; whether a clip's taps are read from LDS or through the cache is decided per table, and the dynamic LDS is
 * sized for the largest LDS-resident table of the launch.
 * Limits (DS2_ERR_ARG with a text outside them, and nothing is written): B in 1..65535; n_tables in 1..16; per table L in
 * 1..1024, M in 1..4096, K odd in 1..1023, and the table inside the bank; max_out >= 0 (0: nothing is launched).
 * The device cannot report an error, so these are defined instead: a clip whose table id is outside [0, n_tables) or whose
 * length is negative is skipped -- nothing is written for it; outputs at or past max_out of a clip are not written.
 * Added without a change of DS2_ABI_VERSION: one new symbol, no existing signature altered. */
#define DS2_RESAMPLE_VAR_TABLES 16
typedef struct ds2_resample_table {
    int32_t L, M, K;
    int32_t tap_offset;                                           /* in floats, into tap_bank */
} ds2_resample_table;
int ds2_resample_var(const int16_t* pcm, const int64_t* in_offsets, const int64_t* out_offsets, const int32_t* table_ids, int B,
                     const ds2_resample_table* tables_host, int n_tables, const float* tap_bank, size_t bank_floats, int max_out,
                     int16_t* out, void* stream);

/* ------------------------------------------------------------------ SpecAugment
 * Time warp, frequency masks and time masks on the log-spectrogram of a minibatch, one launch, between ds2_spectrogram_fwd and
 * the model.  The reference has no such stage (its augmentation is tempo, gain and noise, all on the waveform): nothing here is
 * parity, every rule is a decision written down below.
 *   x, out         (B, t_max, 161) float32, the layout ds2_spectrogram_fwd writes
 *   frames         (B) int32: T_b, the clip's valid frames, 1 <= T_b <= t_max (clamped into [0, t_max])
 *   warp           (B, 2) int32: c, c2, both in [0, T_b) (clamped into it) -- or NULL: no clip is warped
 *   fmask, MF      (B, MF, 2) int32: f0, f -- bins [f0, f0 + f) of every valid frame; width f <= 0: no mask
 *   tmask, MT      (B, MT, 2) int32: t0, t -- frames [t0, t0 + t); width t <= 0: no mask
 * Time warp (only with warp != NULL): source frame c lands on output frame c2 and both halves are resampled linearly along
 * time.  For output frame t < c2: num = t * c, den = c2, base = 0; for t >= c2: num = (t - c2) * (T_b - c), den = T_b - c2,
 * base = c.  i0 = base + num / den (integer division), frac = (float)(num % den) / (float)den (one correctly rounded division
 * of two integers below 2^24), i1 = min(i0 + 1, T_b - 1), and y[t][k] = fmaf(frac, x[i1][k] - x[i0][k], x[i0][k]): three
 * float roundings.  Where frac == 0 the kernel stores x[i0][k] itself and does not read x[i1], so c2 == c is the identity bit
 * for bit (a negative zero and a non-finite neighbour included); a clip that is not to be warped is sent as that.  With
 * warp != NULL every T_b must be <= 4096, so that num stays exact in float.
 * Masks are applied to the warped frames, frequency first and then time; overlaps are harmless.  A cell (t, k) with t < T_b
 * becomes mask_value if f0 <= k < f0 + f for any frequency mask or t0 <= t < t0 + w for any time mask.  The value is STORED,
 * never multiplied in: a NaN or inf under a mask comes out as mask_value (the cell is not even read).  Masks are clamped into
 * [0, 161) and [0, T_b): nothing outside the clip's frames is masked.
 * Padding: frames t >= T_b are zero in out, whatever mask_value is.
 * out == x (in place) is allowed only when warp == NULL: the kernel then stores the masked cells only and reads nothing (x's
 * padding is what it was).  Otherwise out must not overlap x (refused), every cell of out is written, padding included, and
 * out need not be initialised; warp == NULL with a separate out is a copy with masks.
 * DS2_ERR_ARG before any launch: x, out or frames NULL; B outside 1..65535; t_max < 1; MF or MT outside 0..8; a NULL table with
 * a non-zero count; x and out overlapping unless they are equal and warp == NULL.  All three tables NULL with MF == MT == 0 is
 * not an error: in place the call returns at once, there is nothing to do.  frames and the tables are device data: the
 * kernel clamps every entry (no entry can make it read or write outside the two buffers); a host wrapper validates them
 * (T_b <= 4096 with a warp, c and c2 in range) before upload.
 * No workspace, no atomics, no cell written twice: a clip's result does not depend on its position in the batch, on the other
 * clips, on t_max, or on what out held before.
 * Added without a change of DS2_ABI_VERSION: one new symbol, no existing signature altered. */
int ds2_spec_augment(const float* x, float* out, int B, int t_max, const int32_t* frames, const int32_t* warp,
                     const int32_t* fmask, int MF, const int32_t* tmask, int MT, float mask_value, void* stream);

/* ------------------------------------------------------------------ generic fp32 GEMM (MFMA)
 * C[M,N] = op(A) * op(B) + beta * C, row-major with leading dimensions.  op(A)=A (M x K, lda) or
 * A^T (A stored K x M); op(B)=B (K x N, ldb) or B^T (B stored N x K).  beta is 0 or 1.
 * Stands in for the cuBLAS calls behind nn.Linear / nn.GRU's input projection
 * (codes/model.py:51-52,178-180).  split_k > 1 splits K over workgroups and accumulates the
 * partial products with float atomics (C is zero-filled first when beta = 0; the last bits then
 * depend on arrival order); split_k = 0 picks a split that fills the chip when M*N alone gives
 * fewer than ~384 tiles (the dW = dG^T X products: small M*N, K = T*B).
 *
 * Arithmetic.  Operands, accumulator and result are fp32.  Two kernel families compute the products:
 *   mode 0      the f32-input matrix instruction (v_mfma_f32_32x32x2_f32): an fp32 FMA chain;
 *   mode 6 / 9  every fp32 operand element is split without error into three bf16 terms a = a1 + a2 + a3
 *               (round-to-nearest at each step: the three 8-bit significands carry all 24 bits), and a * b is summed from
 *               partial products ai * bj on the bf16 matrix instruction, each exact in its fp32 accumulator.  Mode 9 adds
 *               all nine; mode 6 (the default) leaves out a2 b3 + a3 b2 + a3 b3: at most 2^-24.2 |a b| and 6e-9 rms over 10^6 random
 *               products (tests/test_split_cpu.py), where a correctly rounded fp32 multiply is off by up to 2^-24 and 2.5e-8 rms -- less than one fp32
 *               rounding.  Measured against fp64 the three agree to the last digit shown (tools/gemm_split_check.py:
 *               max error / sum|a||b| 2.9e-7 at K = 672 in modes 6 and 9, 3.2e-7 in mode 0).  Not handled like mode 0:
 *               an operand element beyond bf16's largest finite value (3.39e38) or an infinity gives NaN, and terms below
 *               2^-126 are flushed (operands below ~2^-108 lose low bits).
 * ds2_gemm_split_mode(mode) selects the family for later calls (0, 6 or 9; anything else only queries) and returns the one
 * in effect; the process default is DS2_GEMM_SPLIT or 6.  Mode 6 / 9 needs 16-byte aligned operands with leading dimensions
 * that are multiples of 4 and, for an operand stored with K contiguous, K % 16 == 0; other calls use mode 0's kernels.
 */
int ds2_gemm_split_mode(int mode);
int ds2_gemm_f32(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B,
                 int ldb, float* C, int ldc, float beta, int split_k, void* stream);
/* Up to four TN problems C_p[M_p, N] = A_p^T B_p that share N and K in ONE launch (A_p stored K x M_p with leading
 * dimension lda_p, B_p stored K x N): the four weight-gradient GEMMs dW_hh of a BiGRU layer -- two directions x
 * {r|z rows, n rows} of dGH^T h_prev, codes/model.py:51-52's backward -- which as separate launches are too small to fill
 * the chip.  The pointer / size arrays are HOST arrays of `count` entries holding device pointers; K is split over
 * workgroups and accumulated with float atomics into C -- zero-filled by the call, or, with accumulate != 0, added to what
 * C holds (the caller zeroed the whole flat gradient with one fill: C += A^T B). */
int ds2_gemm_f32_tn_group(int count, const float* const* A_host, const int* lda_host, const int* M_host,
                          const float* const* B_host, const int* ldb_host, float* const* C_host, const int* ldc_host,
                          int N, int K, int accumulate, void* stream);

/* ------------------------------------------------------------------ conv stack
 * Replaces nn.Conv2d at codes/model.py:143-144 (cuDNN).  Layouts are NCHW with time innermost:
 *   conv1: x_t (B,161,T_in) [the transposed input, codes/model.py:184] -> y (B,32,61,T1)
 *          kernel (32,1,41,11), stride (2,2), padding (0,10)
 *   conv2: a1 (B,32,61,T1) -> y (B,32,21,T); kernel (32,32,21,11), stride (2,1), no padding
 * which = 1 or 2.  Weights are passed in the torch layout (Cout,Cin,KF,KT) plus bias (32).
 * wt_ws: workspace of ds2_conv_wt_ws_floats(which) floats for the re-laid-out filter.  ds2_conv2_dgrad takes its workspace
 * WITH its size: ds2_conv2_dgrad_ws_floats(B, T1) floats let it choose its gather form, which keeps a zero-bordered copy of
 * d_out there (several million floats); with fewer -- but at least ds2_conv_wt_ws_floats(2) -- it runs the direct kernel;
 * with fewer than that it returns DS2_ERR_ARG.  It never writes past ws_floats.
 * Arithmetic of conv2's forward pass and data gradient: fp32 operands, accumulator and result; by default the products run
 * on the bf16 matrix pipe after the error-free three-way operand split described at ds2_gemm_f32 (six exact partial
 * products; DS2_CONV_SPLIT=9 all nine, =0 the direct kernels on the f32-input matrix instruction; the data gradient takes
 * that form from B * T1 >= 1000 input columns, DS2_CONV_SPLIT_DGRAD=0 / 1 forces a choice).
 * ds2_conv_fwd and ds2_conv_wgrad return DS2_ERR_ARG unless t_in_frames > 0 (conv2: > 10), ds2_conv2_dgrad unless T1 > 10.
 */
int ds2_transpose_btf_to_bft(const float* x, int B, int T, int F, float* x_t, void* stream);
size_t ds2_conv_wt_ws_floats(int which);
int ds2_conv_fwd(int which, const float* in, const float* weight, const float* bias, int B, int t_in_frames,
                 float* out, float* wt_ws, void* stream);
/* dgrad (conv2 only): d_in (B,32,61,T1) from d_out (B,32,21,T) */
size_t ds2_conv2_dgrad_ws_floats(int B, int T1);
int ds2_conv2_dgrad(const float* d_out, const float* weight, int B, int T1, float* d_in, float* wt_ws,
                    size_t ws_floats, void* stream);
/* wgrad: d_weight (Cout,Cin,KF,KT) and d_bias (32) OVERWRITTEN (d_weight zeroed inside) */
int ds2_conv_wgrad(int which, const float* in, const float* d_out, int B, int t_in_frames, float* d_weight,
                   float* d_bias, void* stream);

/* ------------------------------------------------------------------ BatchNorm
 * BatchNorm2d(32)+Hardtanh(0,20) of codes/model.py:143-145 on (B,C,D,T) and the sequence-wise
 * BatchNorm1d of codes/model.py:27-34,50,59-60,178 on (rows=T*B, F) -- both including padded
 * frames, eps 1e-5, momentum 0.1, running_var fed the unbiased estimate.
 *
 * Training: *_stats computes batch mean / biased var into stat[0:C], stat[C:2C] (=mean, invstd
 * after finalisation) and updates running_mean/var; *_apply normalises.  Eval: pass
 * use_running=1 to *_stats to derive mean/invstd from the running buffers instead.
 * ws: >= ds2_bn_ws_bytes(C) bytes.
 * running_mean and running_var come as a pair: both NULL (training without a buffer update) or both set; one
 * without the other is DS2_ERR_ARG.
 * Limits (a launch's grid.y; beyond them DS2_ERR_ARG, nothing is launched): ds2_bn2d_stats C <= 65535;
 * ds2_bn2d_apply_htanh B*C <= 65535 with layout_tbf=0, B <= 65535 with layout_tbf=1; ds2_bn2d_htanh_bwd B*C <= 65535.
 */
size_t ds2_bn_ws_bytes(int C);
/* conv flavour, x (B,C,inner) with inner = D*T */
int ds2_bn2d_stats(const float* x, int B, int C, int inner, float eps, float momentum, int use_running,
                   float* running_mean, float* running_var, float* mean_invstd, void* ws, void* stream);
/* y = hardtanh(bn(x), 0, 20); layout_tbf=0: y (B,C,inner); layout_tbf=1 (conv2 -> GRU input, fuses
 * codes/model.py:189-192): x (B,C,D,T) -> y (T,B,C*D) */
int ds2_bn2d_apply_htanh(const float* x, const float* mean_invstd, const float* gamma, const float* beta,
                         int B, int C, int D, int T, int layout_tbf, float* y, void* stream);
/* backward of the above: dy (B,C,D,T) [a (T,B,C*D) gradient is first brought back with
 * ds2_transpose2d(dy, T, B*C*D)] -> dx (B,C,D,T); dgamma,dbeta (C) overwritten */
int ds2_bn2d_htanh_bwd(const float* x, const float* dy, const float* mean_invstd, const float* gamma,
                       const float* beta, int B, int C, int D, int T, float* dx, float* dgamma,
                       float* dbeta, void* ws, void* stream);
/* sequence flavour.  x = xa (+ xb if xb != NULL): the sum of the two GRU directions
 * (codes/model.py:64-67) is folded into the BN read.  rows = T*B. */
int ds2_bn1d_stats(const float* xa, const float* xb, int rows, int F, float eps, float momentum,
                   int use_running, float* running_mean, float* running_var, float* mean_invstd, void* ws,
                   void* stream);
int ds2_bn1d_apply(const float* xa, const float* xb, const float* mean_invstd, const float* gamma,
                   const float* beta, int rows, int F, float* y, void* stream);
/* dx (rows,F) = BN backward of dy; x recomputed from xa(+xb).  dgamma, dbeta overwritten. */
int ds2_bn1d_bwd(const float* xa, const float* xb, const float* dy, const float* mean_invstd,
                 const float* gamma, int rows, int F, float* dx, float* dgamma, float* dbeta, void* ws,
                 void* stream);
/* Segmented sequence flavour (ABI revision 403): the G <= 8 per-task heads of the multi-task model
 * (codes/model.py:210-253), one launch per stage for all G tasks.  x = xa (+ xb) is (T,B,F); task g owns the
 * batch columns [bounds[g], bounds[g+1]) (bounds_host: G + 1 host ints, 0 = bounds[0] < ... < bounds[G] = B), so
 * its rows t*B + b are strided.  Each task is normalised over its own T*B_g rows (padded frames included), as the
 * reference's per-head BatchNorm1d on x[:, b0:b1].  The *_host arguments are host arrays of G device pointers.
 * mean_invstd: (G, 2F), task g's mean then invstd.  ws: >= G * ds2_bn_ws_bytes(F) bytes.
 * stats: training (use_running=0) updates each task's running_mean / running_var (both arrays may be NULL: no update);
 * use_running=1 reads them instead.
 * Limit: T * B <= INT_MAX (the kernels index rows in int); beyond it DS2_ERR_ARG, nothing is launched. */
int ds2_bn1d_seg_stats(const float* xa, const float* xb, int T, int B, int F, int G, const int* bounds_host,
                       float eps, float momentum, int use_running, float* const* running_mean_host,
                       float* const* running_var_host, float* mean_invstd, void* ws, void* stream);
/* y PACKED (T*B, F): task g's rows form the contiguous (T, B_g, F) block at row T*bounds[g]. */
int ds2_bn1d_seg_apply(const float* xa, const float* xb, const float* mean_invstd, int T, int B, int F, int G,
                       const int* bounds_host, const float* const* gamma_host, const float* const* beta_host,
                       float* y, void* stream);
/* dxf PACKED as ds2_bn1d_seg_apply's y -> dy interleaved (T,B,F), every element written (the segments cover B);
 * each task's dgamma, dbeta (F) overwritten. */
int ds2_bn1d_seg_bwd(const float* xa, const float* xb, const float* dxf, const float* mean_invstd, int T, int B,
                     int F, int G, const int* bounds_host, const float* const* gamma_host, float* dy,
                     float* const* dgamma_host, float* const* dbeta_host, void* ws, void* stream);

/* ------------------------------------------------------------------ bidirectional GRU recurrence
 * Replaces nn.GRU(bias=False, bidirectional=True) (codes/model.py:51-52,62) -- the cuDNN RNN.
 * The input projection gi = X W_ih^T is a ds2_gemm_f32 call made by the caller into G.
 *   G     (T,B,2,3H)  in: gi (gate order r,z,n; dir 0 forward, dir 1 reverse)
 *                     out: the gate activations r,z,n (saved for backward)
 *   ghn   (T,B,2,H)   out: W_hn h_{t-1} (saved for backward)
 *   hout  (2,T,B,H)   out: hidden state of each direction at every step; h_0 = 0; the reverse
 *                     direction runs t = T-1 .. 0 over the PADDED length (no packing, :62)
 *   w_hh  (2,3H,H)    both directions' recurrent weights, dir-major
 * The caller sums hout[0]+hout[1] (codes/model.py:64-67) inside the next BN read.
 */
int ds2_gru_bidir_fwd(float* G, float* ghn, float* hout, const float* w_hh, int T, int B, int H,
                      void* stream);
/* BPTT.  d_out (T,B,H) is the gradient w.r.t. the direction SUM (so it feeds both directions).
 *   G     in: r,z,n  out: d(gi) = [dr_pre, dz_pre, dn_pre]      (T,B,2,3H)
 *   ghn   in: W_hn h  out: d(gh_n) = dn_pre * r                  (T,B,2,H)
 *   w_hh_t (2,H,3H)   transposed recurrent weights (ds2_transpose2d per direction)
 *   dh_ws  workspace of 2*2*B*H floats
 */
int ds2_gru_bidir_bwd(float* G, float* ghn, const float* hout, const float* d_out, const float* w_hh_t,
                      float* dh_ws, int T, int B, int H, void* stream);
int ds2_transpose2d(const float* in, int rows, int cols, float* out, void* stream);
/* The same for `count` (<= 8) separately placed inputs of `batch` row-major (rows, cols) matrices each, in ONE launch:
 * in_host = HOST array of `count` device pointers; out = (count, batch, cols, rows).  The training forward pass transposes the
 * recurrent weights of all five layers (two directions each, adjacent in the flat parameter buffer) for the backward recurrence
 * with one call instead of ten (ABI revision 402). */
int ds2_transpose2d_group(int count, const float* const* in_host, int batch, int rows, int cols, float* out, void* stream);
/* Persistent form of the two calls above: ONE launch per layer pass; every workgroup keeps its slice
 * of the recurrent weights in registers for all T steps and hands h_t (forward) / d(gh)_t (backward)
 * to the other workgroups of its direction (and batch part) inside the launch: write-through stores
 * into an exchange ring inside sync_ws, one arrival add per workgroup per step on sharded counters,
 * one polling wave per consumer, write-through-coherent loads straight into MFMA operands.  The form
 * (4x4x1 or 16x16x4 MFMA, 1-3 batch parts) is chosen from B and H; results do not depend on it beyond
 * fp32 summation order.  Same arguments and results as the per-step calls; sync_ws is a caller-owned
 * device buffer of ds2_gru_sync_ws_bytes(B, H) bytes, 16-byte aligned, that the CALLER ZEROES ONCE
 * when it allocates it: a launch that completes leaves its counters zero for the next one (the last
 * workgroup to leave resets them), so no memset runs between launches.  Every spin is bounded (5 s):
 * on a timeout the 32-bit word at byte offset ds2_gru_sync_error_offset() of sync_ws is set to 1 and
 * the launch ends.  EVERY output of a launch that sets the word -- G, ghn, hout and the exchange ring -- is UNDEFINED: the
 * step in which the time-out happened still publishes a payload computed from the missing fragment and stores its
 * activations before the workgroups return.  The word is STICKY -- later launches never clear it --
 * so one check after synchronising at the end of a step covers every launch of the step; after a
 * reported timeout the caller zeroes the whole workspace before using it again.
 * All workgroups of a launch must be resident at once: ds2_gru_persistent_supported(B, H) answers for
 * the CURRENT device from its compute-unit count (grid <= 15/16 of the CUs, so a concurrent RCCL
 * kernel keeps some) and the shape limits (H % 16 == 0, B <= 64); the launch itself re-checks the
 * chosen kernel with hipOccupancyMaxActiveBlocksPerMultiprocessor.  DS2_ERR_UNSUPPORTED = use the
 * per-step calls above instead (partitioned or smaller devices). */
size_t ds2_gru_sync_ws_bytes(int B, int H);
size_t ds2_gru_sync_error_offset(void);
int ds2_gru_persistent_supported(int B, int H);
int ds2_gru_bidir_fwd_persistent(float* G, float* ghn, float* hout, const float* w_hh, void* sync_ws, int T,
                                 int B, int H, void* stream);
int ds2_gru_bidir_bwd_persistent(float* G, float* ghn, const float* hout, const float* d_out,
                                 const float* w_hh_t, void* sync_ws, int T, int B, int H, void* stream);
/* The same with a hint (ABI revision 401): spare_cus = compute units the caller wants left FREE beside this launch for work
 * it has queued on other streams (the weight-gradient GEMMs of the layer above, a collective); < 0 = the library's default.
 * For B = 9 .. 12 the kernel exists with 20, 24 or 28 hidden units per workgroup (240 / 204 / 174 workgroups at H = 800;
 * 2.65 / 2.82 / 3.0 us per time step stand-alone at B = 10): the launch takes the widest grid that leaves spare_cus free.
 * Same results, same workspace; elsewhere the hint is ignored. */
int ds2_gru_bidir_bwd_persistent_ex(float* G, float* ghn, const float* hout, const float* d_out,
                                    const float* w_hh_t, void* sync_ws, int T, int B, int H, int spare_cus, void* stream);
/* The d(h) hand-off form of the backward recurrence (ABI revision 402; the reference: cuDNN's GRU backward under
 * codes/model.py:51-52,62).  d(gh)_t[b, g, j] = dh_t[b, j] * c_g[t, b, j], where the three coefficient planes
 *     c_r = (1 - z)(1 - n^2) gh_n r (1 - r),   c_z = (h_prev - n) z (1 - z),   c_n = (1 - z)(1 - n^2) r
 * depend on the forward pass's saved activations only.  With `coef` (T, B, 2, 3H) = (c_r | c_z | c_n) per (t, b, direction)
 * row given, the workgroups hand off dh_t (H values per batch row and step) instead of d(gh)_t (3H) and rebuild d(gh) at
 * the consumer from coefficient fragments loaded a step ahead.  Same inputs / outputs / workspace / error contract as
 * ds2_gru_bidir_bwd_persistent_ex; results equal up to fp32 rounding of the re-associated products.
 *   ds2_gru_bwd_coef:          coef from G (= r, z, n), ghn, hout as ds2_gru_bidir_fwd* left them (an elementwise pass)
 *   ds2_gru_bwd_dh_supported:  1 where the form is built (H = 800, 5 <= B <= 12; H = 64 for tests), else 0 -- the caller
 *                              then uses ds2_gru_bidir_bwd_persistent_ex; the launch itself returns DS2_ERR_UNSUPPORTED */
int ds2_gru_bwd_dh_supported(int B, int H);
/* ds2_gru_bidir_fwd_persistent with the coefficient planes as a fourth output: coef (T, B, 2, 3H) or NULL.  Where the forward
 * form that runs can (B = 9 .. 12 at H = 800) its own gate threads write them; otherwise ds2_gru_bwd_coef runs behind the
 * launch on the same stream.  A training forward pass that will call ds2_gru_bidir_bwd_persistent_dh asks for them here. */
int ds2_gru_bidir_fwd_persistent_ex(float* G, float* ghn, float* hout, const float* w_hh, float* coef, void* sync_ws, int T,
                                    int B, int H, void* stream);
int ds2_gru_bwd_coef(const float* G, const float* ghn, const float* hout, float* coef, int T, int B, int H, void* stream);
int ds2_gru_bidir_bwd_persistent_dh(float* G, float* ghn, const float* hout, const float* d_out, const float* w_hh_t,
                                    const float* coef, void* sync_ws, int T, int B, int H, int spare_cus, void* stream);

/* ------------------------------------------------------------------ output head helpers
 * softmax over the last dim of (rows, A) (eval branch, codes/model.py:204-205) and the argmax
 * of GreedyDecoder.decode (codes/decoder.py:154; ties -> lowest index, NaN counts as the largest value and the first
 * one wins, as torch.max: the index is always in [0, A)). */
int ds2_softmax_rows(const float* x, int rows, int A, float* y, void* stream);
int ds2_argmax_rows(const float* x, int rows, int A, int32_t* idx, void* stream);
/* greedy collapse on device: best (B,T) int32 (batch-major), sizes (B) -> out_ids (B,T) and
 * out_offsets (B,T) compacted per row, out_lens (B)   (codes/decoder.py:123-140) */
int ds2_greedy_collapse(const int32_t* best, const int32_t* sizes, int B, int T, int blank,
                        int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens, void* stream);

/* ------------------------------------------------------------------ host-side scoring / decoding helpers
 * HOST pointers, no stream.
 * ds2_edit_distance: Levenshtein distance of two int32 sequences (>= 0; negative = error).  Replaces the
 *   python-Levenshtein calls under Decoder.wer / Decoder.cer (codes/decoder.py:20,49-78).
 * ds2_ctc_beam_search: CTC prefix beam search over ONE utterance's (T, A) probabilities (log_input = 0) or
 *   log-probabilities (log_input = 1); writes the best labelling (<= out_cap labels), the frame each label first
 *   appeared at, its length and log-probability.  Not in the reference (test.py:21 offers greedy / none only);
 *   SURVEY.md 8f rank 4. */
int ds2_edit_distance(const int32_t* a, int na, const int32_t* b, int nb);
int ds2_ctc_beam_search(const float* probs, int T, int A, int blank, int beam_width, int log_input,
                        int32_t* out_labels, int32_t* out_offsets, int out_cap, int* out_len, float* out_logp);

/* ------------------------------------------------------------------ device CTC beam search (csrc/ctc_beam.hip)
 * Not in the reference.  One launch decodes a batch: probs (B,T,A) on the device, probabilities (log_input = 0) or
 * log-probabilities (log_input = 1), sizes (B) int32 frames per utterance (clamped to 0..T).  Same prefix rules as
 * ds2_ctc_beam_search, fp64 accumulation, ranked by log(p_b + p_nb) + alpha * LM + beta * N; ties -> lower candidate
 * index (slot * A + symbol), so a run is bit-reproducible.  1 <= beam_width <= 128, A <= 128.
 * LM (unit 0 = none: the LM arguments are ignored; 1 = char; 2 = word): ngram_table = (ngram_cap, 2) uint64 entries of
 * codes/lm.py (key = ds2_hash of the token ids, payload = float ln p | float ln backoff << 32), order 1..8; word mode
 * adds word_table (word_cap, 2) = hash of a word's alphabet indices -> word id, and space_id = the space label.
 * bos_id / eos_id = the ids of <s> / </s>, unk_id = the id an out-of-vocabulary token enters the history as; it scores
 * oov_logp (natural log).  ws >= ds2_ctc_beam_ws_bytes(B, T, beam_width) bytes (the per-utterance node arrays).
 * Outputs: out_labels / out_offsets (B,T) int32 (the best labelling and the frame each label was appended at on its
 * surviving lineage; zero past out_len), out_len (B), out_score (B) the fused score with the end-of-utterance terms,
 * out_ctc_logp (B) log(p_b + p_nb) of the best labelling. */
size_t ds2_ctc_beam_ws_bytes(int B, int T, int W);
int ds2_ctc_beam_search_batch(const float* probs, const int32_t* sizes, int B, int T, int A, int blank,
                              int beam_width, int log_input, const void* ngram_table, int ngram_cap,
                              const void* word_table, int word_cap, int order, int unit, int bos_id, int eos_id,
                              int unk_id, int space_id, float alpha, float beta, float oov_logp, void* ws,
                              size_t ws_bytes, int32_t* out_labels, int32_t* out_offsets, int32_t* out_len,
                              float* out_score, float* out_ctc_logp, void* stream);

/* ds2_ctc_beam_search_rows: the batch search with R output rows decoupled from the B utterances, for sweeps over the LM
 * weights: many (alpha, beta) pairs over the same probabilities in ONE launch (one workgroup per row).  Row r decodes
 * utterance utt[r] (R int32 on the device) with alpha[r] / beta[r] (R float32 on the device; not read when unit = 0) into
 * row r of out_labels / out_offsets (R,T) and out_len / out_score / out_ctc_logp (R).  Every other argument is as for
 * ds2_ctc_beam_search_batch; ws >= ds2_ctc_beam_ws_bytes(R, T, beam_width).
 * Row r equals, bit for bit, what ds2_ctc_beam_search_batch writes for utterance utt[r] with (alpha[r], beta[r]) -- labels,
 * offsets, length, both scores and the zeros past the length (each float weight becomes a double once, as there) -- and
 * does not depend on which other rows share the launch.  A utt[r] outside [0, B) is checked on the device: that row is the
 * empty labelling with out_score = out_ctc_logp = -inf, and nothing of probs or sizes is read for it.
 * R = 0 is DS2_OK; a bad size or a NULL pointer is DS2_ERR_ARG with a message, as for the batch entry.
 * Added without a change of DS2_ABI_VERSION: one new symbol, no existing signature altered. */
int ds2_ctc_beam_search_rows(const float* probs, const int32_t* sizes, const int32_t* utt, const float* alpha,
                             const float* beta, int B, int R, int T, int A, int blank, int beam_width, int log_input,
                             const void* ngram_table, int ngram_cap, const void* word_table, int word_cap, int order,
                             int unit, int bos_id, int eos_id, int unk_id, int space_id, float oov_logp, void* ws,
                             size_t ws_bytes, int32_t* out_labels, int32_t* out_offsets, int32_t* out_len,
                             float* out_score, float* out_ctc_logp, void* stream);

/* ds2_ctc_beam_search_bias: the batch search with phrase boosting (a context graph over a list of phrases).
 * The rule ("phrase boosting"; a decision of this project).  Phrases are label sequences of 1..DS2_BIAS_MAX_LEN labels
 * without the blank and without duplicates, at most DS2_BIAS_MAX_PHRASES of them; the trie of all their prefixes has at most
 * DS2_BIAS_MAX_STATES nodes, root included.  For a label sequence y two integers are defined by a LEFTMOST-LONGEST,
 * NON-OVERLAPPING scan.  Start with i = 0, m = 0 and repeat while i < len(y):
 *   pending (V only)  if y[i:] is a node of the trie (a prefix of some phrase, complete or not), stop with
 *                     V(y) = m + len(y) - i: a credit that is revocable;
 *   otherwise         let l be the length of the longest phrase that is a prefix of y[i:]; if l > 0, m += l and i += l, else
 *                     i += 1.
 * If the loop ends without stopping, V(y) = m.  F(y) is the same scan without the pending rule: at every i it takes the
 * longest complete phrase or steps by one, so F(y) is the number of labels of y covered by the chosen occurrences.
 * The search ranks a prefix by  log(p_b + p_nb) + alpha * LM + beta * N + w * V(prefix);  at the end of the utterance w * F
 * takes the place of w * V.  w = bias_weight, one float32 per matched label in nats, becomes a double once.  So a prefix
 * earns credit label by label while it spells a phrase and loses the part that never became a complete phrase the moment
 * it leaves the phrase: with NEW and NEW YORK boosted, NEW YOLK keeps 3, not 7.
 * The scan is a deterministic automaton over the trie's nodes, since only the pending string can influence later
 * decisions.  Nodes are numbered in BFS order, children in ascending label order, root = 0:
 *   bias_trans (S, A) int32 on the device: entry [s][c] = next node (low 16 bits) | gain << 16 (high 16 bits, signed) with
 *              gain = V(path(s) + c) - depth(s), in -63..+1.  The blank column is never read.
 *   bias_final (S) int32: final[s] = F(path(s)) - depth(s) <= 0.
 * Summing the gains along y gives V(y); adding final of the state reached gives F(y).  V and F stay integers in the
 * kernel: every beam entry carries (state, count), both functions of the prefix alone (so merging stays sound), and the
 * score term is w * (double)count, added after log p + acc, without fused multiply-adds: the bias never accumulates
 * rounding.  At the end of the utterance w * (double)(count + final[state]) is added to the LM end terms.  The tie rules are
 * those of ds2_ctc_beam_search_batch.
 * S = bias_states, 1 <= S <= DS2_BIAS_MAX_STATES.  A next node outside [0, S) is taken as the root (checked on the device):
 * a malformed table can give a wrong answer but never an out-of-range read.  out_bias (B) int32 = count + final[state] of
 * the returned labelling (0 for the empty beam of an impossible input).  Every other argument and output is as for
 * ds2_ctc_beam_search_batch, and so are its refusals; S out of range, a NULL table or out_bias, or a weight that is not
 * finite are DS2_ERR_ARG with a message before any HIP call.  A root-only graph (S = 1, gains 0) or a weight of 0 gives the
 * labels, offsets, lengths and scores of ds2_ctc_beam_search_batch.
 * Added without a change of DS2_ABI_VERSION: one new symbol, no existing signature altered. */
#define DS2_BIAS_MAX_LEN 64
#define DS2_BIAS_MAX_PHRASES 1024
#define DS2_BIAS_MAX_STATES 32768
int ds2_ctc_beam_search_bias(const float* probs, const int32_t* sizes, int B, int T, int A, int blank,
                             int beam_width, int log_input, const void* ngram_table, int ngram_cap,
                             const void* word_table, int word_cap, int order, int unit, int bos_id, int eos_id,
                             int unk_id, int space_id, float alpha, float beta, float oov_logp,
                             const int32_t* bias_trans, const int32_t* bias_final, int bias_states, float bias_weight,
                             void* ws, size_t ws_bytes, int32_t* out_labels, int32_t* out_offsets, int32_t* out_len,
                             float* out_score, float* out_ctc_logp, int32_t* out_bias, void* stream);

/* ds2_ctc_beam_search_nbest: the batch search that returns the N best entries of its final beam, not one.
 * Same search.  Frame by frame this is the search of ds2_ctc_beam_search_batch and, with a non-NULL bias_trans, that of
 * ds2_ctc_beam_search_bias: the beam, the merging, the LM and bias terms, the fp64 scores and the tie rules at the cut are
 * theirs.  Only the end differs.
 * Valid entries.  After the last frame slot i of the final beam has its end-adjusted score v_i = log(p_b + p_nb) + the LM
 * terms with the end-of-utterance ones + w * F, the number the 1-best entries pick by.  Slot i is VALID if v_i > -1e300, the
 * condition under which that pick can choose it; a NaN is not valid.
 * Ranking.  rank_i = #{valid j : v_j > v_i} + #{valid j < i : v_j == v_i}: a higher score comes first, an exact tie goes to
 * the lower slot.  out_count[b] = min(nbest, number of valid slots).
 * Rows.  Outputs have nbest rows per utterance: out_labels / out_offsets (B,N,T) int32, out_len (B,N) int32, out_score /
 * out_ctc_logp (B,N) float32, out_bias (B,N) int32, out_count (B) int32.  Row n < out_count[b] holds the slot of rank n: its
 * labels, the frame each label was appended at on ITS OWN surviving lineage, its length, (float)v, (float)log(p_b + p_nb)
 * and, with boosting, count + final[state].  Row 0 is bit for bit what the 1-best entry (_batch, or _bias with a graph)
 * writes for that utterance.  Rows n >= out_count[b] have length 0, score and ctc_logp -inf (as the 1-best entries write for
 * an impossible input) and bias 0.  Every row is zero past its length in out_labels and out_offsets.  The rows of one
 * utterance are distinct labellings, since the final beam holds each prefix once (up to the 64-bit hash collision that the
 * merge of csrc/ctc_beam.hip admits).
 * Limits.  1 <= nbest <= beam_width; ws >= ds2_ctc_beam_ws_bytes(B, T, beam_width): the workspace is that of the 1-best
 * entries, whose node arrays already hold every lineage.
 * Refusals, DS2_ERR_ARG with a message before any HIP call: nbest out of range (the message names nbest and beam_width); a
 * NULL output or a NULL out_count; with a non-NULL bias_trans what ds2_ctc_beam_search_bias refuses (states out of range, a
 * NULL bias_final or out_bias, a weight that is not finite); and everything the batch entry refuses, under this function's
 * name.  With bias_trans == NULL there is no boosting: bias_final, bias_states, bias_weight and out_bias are ignored and
 * out_bias is not written.  B = 0 is DS2_OK.
 * Determinism.  Results are bit-identical from run to run and do not depend on the other utterances, on the workspace's
 * contents or on what the outputs held; nothing outside the stated output extents is written.
 * Added without a change of DS2_ABI_VERSION: one new symbol, no existing signature altered. */
int ds2_ctc_beam_search_nbest(const float* probs, const int32_t* sizes, int B, int T, int A, int blank,
                              int beam_width, int log_input, const void* ngram_table, int ngram_cap,
                              const void* word_table, int word_cap, int order, int unit, int bos_id, int eos_id,
                              int unk_id, int space_id, float alpha, float beta, float oov_logp,
                              const int32_t* bias_trans, const int32_t* bias_final, int bias_states, float bias_weight,
                              int nbest, void* ws, size_t ws_bytes, int32_t* out_labels, int32_t* out_offsets,
                              int32_t* out_len, float* out_score, float* out_ctc_logp, int32_t* out_bias,
                              int32_t* out_count, void* stream);

/* ------------------------------------------------------------------ error counts from labels (csrc/edit_stats.hip)
 * Not in the reference (its test.py makes strings and calls python-Levenshtein per utterance).  Word and character error
 * counts of R hypothesis rows against their references in one launch, from label ids; no strings.
 * hyp (R, hyp_stride) int32 and hyp_len (R): the layout ds2_ctc_beam_search_batch / _rows and ds2_greedy_collapse write;
 * nothing past hyp_len[r] is read.  References as for ds2_ctc_loss_grad: flat ref, ref_offsets (N), ref_lens (N), every
 * length <= max_ref_len.  Row r is scored against reference ref_index[r] (R int32), or against reference r if ref_index
 * is NULL.  group (R) int32 in [0, G), or NULL for no totals.  space_id: the space label, -1 = the alphabet has none
 * (labels are >= 0).
 *   items     character level: the sequence with every space_id label removed (Decoder.cer).  Word level: the maximal
 *             runs of non-space labels (str.split(): leading, trailing and repeated spaces make no word); two words are
 *             equal only if they have the same length and the same labels (a hash filters, the labels decide).
 *   distance  unit-cost Levenshtein over hypothesis prefix i and reference prefix j: cell (i, j), 0 <= i <= m, 0 <= j <= n.
 *   counts    every cell takes ONE predecessor and carries that predecessor's (S, D, I) plus its own operation.  Cell
 *             (0, 0) is (0, 0, 0); row i = 0 is all deletions, (0, j) = j D; column j = 0 is all insertions, (i, 0) = i I.
 *             Otherwise, if hypothesis item i equals reference item j the cell takes (i-1, j-1) unchanged (a match, which
 *             is always among the cheapest moves); if not, it takes the cheapest of substitution ((i-1, j-1) + S),
 *             deletion (a reference item without a hypothesis item: (i, j-1) + D) and insertion ((i-1, j) + I), a tie
 *             going to substitution, then deletion, then insertion.  The rule is per cell, so the counts of cell (m, n)
 *             are those of a back-trace from (m, n) under the same rule; no back-pointer is stored.  S + D + I = dist.
 * Outputs: stats (R, 10) int32 = [char_dist, char_sub, char_del, char_ins, ref_chars, word_dist, word_sub, word_del,
 * word_ins, ref_words], ref_chars the reference's non-space labels and ref_words its words.  With group, the ten values of
 * every valid row are ADDED to row group[r] of totals (G, 10) int64: the caller zeroes it (or keeps accumulating); the adds
 * are integer, so the sums do not depend on their order.
 * hyp_stride and max_ref_len <= DS2_EDIT_MAX_ITEMS, else DS2_ERR_ARG.  Checked on the device: a hyp_len[r] outside
 * [0, hyp_stride], a reference index outside [0, N), a ref_lens outside [0, max_ref_len], a group[r] outside [0, G); such
 * a row has -1 in all ten stats and adds nothing to the totals.
 * ds2_edit_stats_ws_bytes(R, hyp_stride, max_ref_len) sizes ws (today 0: the table sweep lives in LDS; ws may then be
 * NULL); its contents never matter.  One workgroup of DS2_EDIT_THREADS threads per (row, level); in the item pass a thread
 * owns DS2_EDIT_CHUNK consecutive labels.  Results are bit-identical from run to run and do not depend on the other rows.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_EDIT_MAX_ITEMS 2048
#define DS2_EDIT_THREADS 256
#define DS2_EDIT_CHUNK (DS2_EDIT_MAX_ITEMS / DS2_EDIT_THREADS)
size_t ds2_edit_stats_ws_bytes(int R, int hyp_stride, int max_ref_len);
int ds2_edit_stats(const int32_t* hyp, const int32_t* hyp_len, int R, int hyp_stride, const int32_t* ref,
                   const int32_t* ref_offsets, const int32_t* ref_lens, int N, int max_ref_len, const int32_t* ref_index,
                   const int32_t* group, int G, int space_id, void* ws, size_t ws_bytes, int32_t* stats, int64_t* totals,
                   void* stream);

/* ------------------------------------------------------------------ CTC forced alignment (csrc/ctc_align.hip)
 * Not in the reference.  One launch finds, for every utterance of a batch, the single best alignment (max-sum / Viterbi) of
 * its KNOWN transcript to frames 0 .. sizes[b]-1, over the extended sequence blank, l1, blank, ..., lL, blank (state s:
 * even = blank, odd = label s/2) with the CTC transitions stay, s-1, and s-2 onto a label that differs from the one at s-2;
 * the path starts in state 0 or 1 and ends in state 2L or 2L-1.  probs (B,T,A) and sizes (B) as for the beam search (sizes
 * clamped to 0..T; nothing past sizes[b] is read, padding may hold NaN); labels / label_offsets / label_lens as for
 * ds2_ctc_loss_grad.  The per-frame term is the input (log_input = 1) or its fp32 log (log_input = 0, log 0 = -inf); a NaN
 * counts as -inf; path scores are carried in fp64.  Ties: at each (t, s) stay wins, then s-1, then s-2; at the end state 2L
 * wins over 2L-1 -- so a result is bit-reproducible and does not depend on the rest of the batch.
 * max_label_len >= every label_lens[b], <= 511 (one state per thread; longer is DS2_ERR_ARG); A <= 256.
 * ws >= ds2_ctc_align_ws_bytes(B, T, max_label_len) bytes (one back-pointer byte per frame and state; need not be zeroed).
 * Outputs: states (B,T) int32 the state index per frame, -1 from sizes[b] on; starts / ends (B,max_label_len) int32 the
 * first and last frame (inclusive) spent in each label's state, -1 past label_lens[b]; score (B) the path's log-score.
 * No alignment (more labels plus adjacent repeats than frames, every path -inf, a label id outside [0, A) or equal to
 * blank, a label_lens[b] outside 0..max_label_len -- checked on the device): score = -inf and states / starts / ends all -1.
 * An empty transcript gives the all-blank path.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
size_t ds2_ctc_align_ws_bytes(int B, int T, int max_label_len);
int ds2_ctc_align(const float* probs, const int32_t* sizes, const int32_t* labels, const int32_t* label_offsets,
                  const int32_t* label_lens, int B, int T, int A, int max_label_len, int blank, int log_input, void* ws,
                  size_t ws_bytes, int32_t* states, int32_t* starts, int32_t* ends, float* score, void* stream);

/* ------------------------------------------------------------------ banded CTC alignment (csrc/ctc_align_banded.hip)
 * Not in the reference.  ds2_ctc_align's quantity -- the same states, transitions, fp64 path scores, per-frame term and tie
 * rule -- restricted to a moving band of W = band states per frame, so that work and workspace are T x W and a recording of
 * an hour aligns to its whole transcript in one launch.  probs (B,T,A), sizes, labels / label_offsets / label_lens, blank,
 * log_input, states (B,T), starts / ends (B,max_label_len) are as for ds2_ctc_align; there is no 511 limit on
 * max_label_len, only 2 max_label_len + 1 < 2^31; A <= 256.  score (B) is FLOAT64 (an hour's path score is about -1e5).
 * lo (B,T) int32 and band, a power of two in DS2_ALIGN_BAND_MIN .. DS2_ALIGN_BAND_MAX: at frame t < sizes[b] the admissible
 * states are { s : lo[b][t] <= s < lo[b][t] + W, s < S = 2 L + 1 }.  The result is that of the full recursion in which
 * v[t][s] is forced to -inf for every inadmissible s: a predecessor outside frame t-1's band counts as -inf, frame 0 starts
 * from the virtual row that admits states 0 and 1 (if they are in its band), and the path must end in S-1 or S-2 inside the
 * last frame's band.  With lo = 0 everywhere and W >= S the result is ds2_ctc_align's, bit for bit.
 * lo must be >= 0, non-decreasing and rise by less than W from one of an utterance's valid frames to the next (consecutive
 * bands share a state); this is checked on the device, and a violation makes THAT utterance "no alignment": score -inf and
 * states / starts / ends all -1, as for a band that leaves no path and for every case ds2_ctc_align reports so.
 * ws >= ds2_ctc_align_banded_ws_bytes(B, T, band) bytes: one back-pointer byte per frame and band slot (state s of frame t
 * is kept in slot s mod W, which names one state of the band); need not be zeroed.
 * Nothing past sizes[b] frames, past an utterance's labels or past its lo row's valid frames is read.  Results are
 * bit-identical from run to run and depend neither on the batch's other utterances nor on the workspace's contents.
 * DS2_ERR_ARG before any launch: band not a power of two or out of range; A, blank, B, T, max_label_len out of range; a
 * workspace that is too small (the message names the needed size); NULL where data would be read.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_ALIGN_BAND_MIN 64
#define DS2_ALIGN_BAND_MAX 8192
size_t ds2_ctc_align_banded_ws_bytes(int B, int T, int band);
int ds2_ctc_align_banded(const float* probs, const int32_t* sizes, const int32_t* labels, const int32_t* label_offsets,
                         const int32_t* label_lens, const int32_t* lo, int B, int T, int A, int max_label_len, int band,
                         int blank, int log_input, void* ws, size_t ws_bytes, int32_t* states, int32_t* starts,
                         int32_t* ends, double* score, void* stream);

/* ------------------------------------------------------------------ banded CTC alignment with gaps (csrc/ctc_align_banded.hip)
 * Not in the reference.  ds2_ctc_align_banded for recordings with stretches the transcript does not cover: the blank states
 * BETWEEN WORDS may absorb a frame whatever the model says about it, at a fixed price below the frame's best symbol.
 * Everything of ds2_ctc_align_banded holds -- the states S = 2 L + 1, their predecessors, the band and its rules, the virtual
 * first row, the end states, the ties, the fp64 sums, "no alignment" -- except the emission of some blank states:
 *   frame values  lp[t][a] is the fp32 term of the existing entry (the input, or its logf unless log_input; NaN counts as
 *                 -inf).  m[t] = max_a lp[t][a], -inf if the row has nothing finite.  f[t] = m[t] - g, ONE fp32 subtraction,
 *                 -inf when m[t] is -inf.  g = gap_penalty, fp32, >= 0; +inf is allowed.
 *   eligibility   state s is eligible if it is a blank (s even) and s == 0, or s == 2 L, or labels[s/2 - 1] == space, or
 *                 labels[s/2] == space.  With space = -1 only the two end blanks are eligible; an empty transcript's one
 *                 state is eligible.
 *   emission      at an eligible state e = f[t], and the frame is a GAP FRAME, if f[t] > lp[t][blank] (strict, in fp32);
 *                 otherwise e = lp[t][blank].  Every other state's emission is unchanged.  The choice depends on (t, s)
 *                 only, never on the path, so the maximum over predecessors and its tie rule are untouched.
 *   outputs       states, starts, ends and the fp64 score as before; the score includes the gap frames' f[t].  gap (B,T)
 *                 uint8: 1 where the returned path's frame is a gap frame, 0 elsewhere below sizes[b], 0 past sizes[b], all 0
 *                 without an alignment.
 *   identity      with g = +inf, states / starts / ends / score are ds2_ctc_align_banded's bit for bit and gap is all zero.
 *                 With g = 0 every eligible state takes the frame's best symbol for free.
 * space: the label id that separates words, or -1.  DS2_ERR_ARG before any launch: g negative or NaN; space outside
 * {-1} u [0, A) or equal to blank; everything ds2_ctc_align_banded refuses.  ws >= ds2_ctc_align_banded_gap_ws_bytes(B, T,
 * band) bytes (the gap flag is a spare bit of the back-pointer byte, so the size is the plain entry's); need not be zeroed.
 * Results are bit-identical from run to run and depend neither on the batch's other utterances nor on the workspace's contents.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
size_t ds2_ctc_align_banded_gap_ws_bytes(int B, int T, int band);
int ds2_ctc_align_banded_gap(const float* probs, const int32_t* sizes, const int32_t* labels, const int32_t* label_offsets,
                             const int32_t* label_lens, const int32_t* lo, int B, int T, int A, int max_label_len, int band,
                             int blank, int space, float gap_penalty, int log_input, void* ws, size_t ws_bytes,
                             int32_t* states, int32_t* starts, int32_t* ends, uint8_t* gap, double* score, void* stream);

/* ------------------------------------------------------------------ keyword search (csrc/ctc_keyword.hip)
 * Not in the reference, so every rule here is this project's decision.  For every utterance b of a batch and every one of K
 * keywords: where was the keyword said, and how far must the model leave its own best path to have said it there.  Each
 * (b, k) pair is independent of every other pair.
 * logp (B,T,A): fp32 LOG-probabilities (the caller takes the log; there is no log_input switch).  sizes (B) clamped to 0..T;
 * nothing past sizes[b] is read, padding may hold NaN.  labels / label_offsets / label_lens (K) as for ds2_ctc_align, one
 * entry per KEYWORD.  min_score (K) float64.
 *   emission   m[t] = max_a logp[t][a], a NaN counting as -inf;  e[t][a] = logp[t][a] - m[t], ONE fp32 subtraction;  e = -inf
 *              where logp is NaN or -inf or the subtraction gives NaN (m[t] = -inf).  So e <= 0, a frame the model's best
 *              path already spends on the wanted symbol costs 0, and scores of spans of different lengths are comparable.
 *   states     S = 2 L - 1: l1, blank, l2, ..., lL; state s is a label if s is even and a blank if s is odd.  An occurrence
 *              starts in l1's state and ends in lL's, so its span is tight.
 *   recursion  in fp64, v[-1][.] = -inf, st[-1][.] = -1.  s >= 1: v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if s is
 *              even and ext[s] != ext[s-2]) + e[t][ext[s]];  s = 0: v[t][0] = max(v[t-1][0], 0) + e[t][l1], the 0 being a
 *              fresh start at frame t.  st[t][s], the start frame of the state's best path, is copied from the chosen
 *              predecessor and is t on a fresh start.  Ties: stay, then s-1, then s-2 (strict > in that order); at state 0
 *              stay wins over a fresh start, so a run of zero-cost first-label frames starts at its first frame.
 *              D[t] = v[t][S-1] with st[t][S-1] is the best occurrence ending at t.  No back-trace, no per-frame workspace.
 *   hits       the candidate (D[t], st[t][S-1], t) counts when D[t] >= min_score[k] (a NaN threshold compares false).  One
 *              streaming pass over t clusters them: with no current hit the candidate becomes it; if the candidate's start
 *              lies after the current hit's end, the current hit is emitted and the candidate becomes current; otherwise
 *              the candidate replaces the current hit if its score is greater, or equal with the same start (which extends
 *              the end across a plateau); any other candidate is dropped.  The current hit is emitted after the last frame.
 *              Hits come out with ascending ends; a hit MAY BEGIN BEFORE THE PREVIOUS ONE ENDS (a better candidate
 *              replaces the current hit whatever its start, and only the FIRST candidate of a cluster was held against the
 *              emitted hit's end).
 * Outputs: hits (B,K,max_hits,2) int32 (start, end) inclusive, -1 past the count; hit_score (B,K,max_hits) float64, -inf past
 * the count; n_hits (B,K) int32 the TRUE count, which may exceed max_hits: the first max_hits are then written and nothing
 * past them is touched.
 * 1 <= L <= DS2_KWS_MAX_LEN; a keyword outside that range, or with a label outside [0, A) or equal to blank, has n_hits = 0
 * for every utterance (checked on the device).  DS2_ERR_ARG before any launch: A outside 1..256; K outside 1..65535;
 * max_hits outside 1..64; blank outside [0, A); B or T negative or B T > 2^25; a NULL pointer; a workspace smaller than
 * ds2_ctc_keyword_search_ws_bytes(B, T) (the message names the needed size).  The workspace holds m, need not be zeroed and
 * is written only below sizes[b].
 * Results are bit-identical from run to run and depend neither on the batch's other utterances, nor on the other keywords,
 * nor on the workspace's contents.  Two launches on the stream (row maxima, search); no workgroup waits on another.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_KWS_MAX_LEN 64
size_t ds2_ctc_keyword_search_ws_bytes(int B, int T);
int ds2_ctc_keyword_search(const float* logp, const int32_t* sizes, const int32_t* labels, const int32_t* label_offsets,
                           const int32_t* label_lens, const double* min_score, int B, int T, int A, int K, int blank,
                           int max_hits, void* ws, size_t ws_bytes, int32_t* hits, double* hit_score, int32_t* n_hits,
                           void* stream);

/* ------------------------------------------------------------------ unit posterior (csrc/ctc_unit.hip)
 * Not in the reference, so every rule here is this project's decision.  How sure is the model of each WORD (or character) of a
 * decoded label row: the probability, under the model's own frame posteriors, that the frames the decoder gave the unit spell
 * exactly that unit.  Acoustic only: no LM, no boost.  Every (row, unit) is independent of every other.
 * probs (B,T,A): fp32 PROBABILITIES (there is no log_input switch).  sizes (B).  labels / offsets (R,stride) and lens (R): the
 * layout ds2_greedy_collapse and the beam searches return (an N-best result viewed as (B N, T)); utt (R) is each row's
 * utterance, NULL meaning row r belongs to utterance r.
 *   units      space_id >= 0 (words): a unit is a maximal run of labels other than space_id -- leading, trailing and repeated
 *              spaces make no unit.  space_id = -1 (characters): every label is its own unit.  Units are numbered in row order.
 *   span       a unit of labels i .. j-1 (L = j - i >= 1) covers the frames o[i] .. o[j-1] INCLUSIVE of its utterance, n of
 *              them: the offsets the decoder reported for its first and last label, so the span is tight.
 *   value      P = the sum, over all CTC alignments pi of the span's n frames that collapse to the unit's labels, of
 *              prod_t probs[utt][o[i] + t][pi_t]: the CTC forward over the S = 2 L + 1 states blank, l1, blank, .., lL, blank
 *              (blanks allowed at both ends) on the sub-matrix of the span.  0 <= P <= 1 for normalised rows, and over all
 *              labellings of the span the values sum to 1.  A frame spent on another symbol costs exactly that symbol's share.
 *   arithmetic linear, fp64: alpha[0][0] = p[0][blank], alpha[0][1] = p[0][l1];  alpha[t][s] = p[t][ext[s]] * (alpha[t-1][s] +
 *              alpha[t-1][s-1] (+ alpha[t-1][s-2] if s is a label state and ext[s] != ext[s-2])).  Every fp32 probability is
 *              converted to double (exact); a NaN or negative one counts as 0.  All alphas of a unit are rescaled together by
 *              an exact power of two whenever they leave 2^-200 .. 2^200 (looked at every 4 frames) and the exponent e is
 *              summed in an integer.  logp = log(alpha[n-1][S-1] + alpha[n-1][S-2]) + e ln 2 in double; P = 0 gives -inf.
 * Outputs, (R,max_units) each: unit_first (index of the unit's first label in its row), unit_len (its label count) int32 and
 * unit_logp float64; past the row's count first = len = -1 and logp = NaN.  n_units (R) int32 is the TRUE count, which may
 * exceed max_units: the first max_units are then written and nothing past them is touched.  A unit of more than
 * DS2_UNIT_MAX_LABELS labels is listed with logp = NaN; dropped (R) int32 counts such units of the row, listed or not.
 * Checked on the device, not an error: a row is INVALID, with n_units = -1, dropped = 0 and no unit, if lens[r] lies outside
 * 0..stride, utt[r] outside [0, B), a label outside [0, A) or equal to blank, or the offsets are not strictly increasing inside
 * [0, min(sizes[utt], T)).
 * DS2_ERR_ARG before any launch: A outside 1..256; blank outside [0, A); space_id outside -1 .. A-1 or equal to blank; R,
 * stride or max_units < 1; B or T < 1 or B T > 2^25; R stride or R max_units > 2^27; a NULL pointer (utt may be NULL); a
 * workspace smaller than ds2_ctc_unit_posterior_ws_bytes(R, stride, max_units) (the message names the needed size).
 * Nothing outside a unit's span, past sizes[utt], or in a row past its lens is read: all of that may hold NaN.  The workspace
 * (each listed unit's first frame and frame count) need not be zeroed.  Results are bit-identical from run to run and depend
 * neither on the other rows, nor on max_units, nor on the workspace's contents.  Two launches on the stream (units, values);
 * no workgroup waits on another, nothing waits on the stream.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_UNIT_MAX_LABELS 64
size_t ds2_ctc_unit_posterior_ws_bytes(int R, int stride, int max_units);
int ds2_ctc_unit_posterior(const float* probs, const int32_t* sizes, int B, int T, int A, const int32_t* labels,
                           const int32_t* offsets, const int32_t* lens, const int32_t* utt, int R, int stride, int space_id,
                           int blank, int max_units, void* ws, size_t ws_bytes, int32_t* unit_first, int32_t* unit_len,
                           double* unit_logp, int32_t* n_units, int32_t* dropped, void* stream);

/* ------------------------------------------------------------------ voice-activity segmentation (csrc/vad.hip)
 * Not in the reference (it cuts its corpora with dataset scripts and sox).  Cuts a recording of any length into the clips the
 * model was trained on, from the int16 samples already on the device.  Integer arithmetic only: a result is exact.
 * pcm: n int16 samples at 16 kHz.  A block is 160 samples (10 ms); nb = ceil(n / 160); block j covers samples
 * [160 j, 160 j + 160), the part at or past n counting as zeros.
 *   1. energies    E[j] = sum of x^2 over block j (64 bits, at most 160 * 2^30);  S[j] = E[j-1] + E[j] + E[j+1], missing
 *                  neighbours counting as 0
 *   2. level bin   bin(S) = S for S < 4; otherwise e = floor(log2 S), bin = 4 e + ((S >> (e - 2)) & 3): quarter-octave steps
 *                  (0.58 .. 0.97 dB), monotone; the largest value is bin(3 * 160 * 2^30) = 155 (DS2_VAD_BINS = 192 bins)
 *   3. threshold   hist = histogram of bin(S[j]) over the recording; floor_bin = the smallest k with hist[0] + .. + hist[k] >
 *                  rank;  thr = min(max(floor_bin + margin_bins, min_bin), max_bin);  raw mask m[j] = bin(S[j]) >= thr
 *                  (max_bin is what lets a recording that is speech throughout still count as speech)
 *   4. close gaps  a maximal run of m = 0 shorter than min_silence blocks with speech on both sides becomes speech; leading
 *                  and trailing silence is never bridged
 *   5. drop blips  on the result of 4, a maximal run of m = 1 shorter than min_speech blocks is removed; 4 is not repeated
 *   6. pad         each remaining run [s, e) becomes [max(0, s - pad), min(nb, e + pad)); 2 pad < min_silence, so padded runs
 *                  never touch
 *   7. split       with h = (max_len + 1) / 2: while e - s > max_len, cut at the c in [s + h, min(s + max_len, e - h)] with
 *                  the smallest S[c] (ties: the smallest c), emit [s, c) and go on with s = c; then emit [s, e).  Every piece
 *                  of a split run has between h and max_len blocks
 *   8. output      the segments in ascending order as [start_block, end_block); at most nb / min(min_speech, h) + 1 of them.
 *                  In samples a segment is [160 start, min(n, 160 end))
 * segs (seg_cap, 2) int32: rows 0 .. min(n_seg, seg_cap) - 1 hold the segments, rows from n_seg up to seg_cap are -1; with
 * n_seg > seg_cap only seg_cap rows are written, nothing past them is touched, and info[0] still holds the true count.
 * info int32[8]: n_seg, floor_bin, thr, the number of speech blocks after step 5, nb, 0, 0, 0.  n = 0: no segment, info all 0.
 * DS2_ERR_ARG before any launch: min_speech < 2; max_len < 4; pad < 0; 2 pad >= min_silence; rank outside 0 .. max(nb - 1, 0);
 * margin_bins, min_bin or max_bin outside 0 .. 191; n >= 2^31; ws_bytes < ds2_vad_segment_ws_bytes(n); seg_cap < 1; a NULL or
 * misaligned pointer (pcm: 2 bytes, any offset inside a tensor; ws: 16; segs, info: 4).
 * Nothing outside pcm[0 .. n) is read.  ws and segs need not be zeroed; the result does not depend on what they held and is
 * bit-identical from run to run (the only atomics are integer adds into the histogram).  Three launches on the stream: block
 * energies (the one pass over the samples, 16 bytes per lane), S / bin / histogram, then steps 3-8 as scans over run
 * boundaries in one workgroup.  No workgroup waits on another.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_VAD_BLOCK 160
#define DS2_VAD_BINS 192
size_t ds2_vad_segment_ws_bytes(size_t n);
int ds2_vad_segment(const int16_t* pcm, size_t n, int rank, int margin_bins, int min_bin, int max_bin, int min_speech,
                    int min_silence, int pad, int max_len, void* ws, size_t ws_bytes, int32_t* segs, int seg_cap,
                    int32_t* info, void* stream);

/* ------------------------------------------------------------------ CTC
 * Replaces warpctc_pytorch.CTCLoss (train.py:179, codes/engine.py:22, codes/metrics.py:51):
 * softmax over A inside, blank 0, costs[b] = -log p(labels_b | acts[:act_lens[b], b]),
 * grad = grad_scale * d(sum_b costs[b]) / d acts (zero for t >= act_lens[b]; zero for an utterance
 * whose alignment is infeasible, whose cost is +inf).  grad_scale carries the 1/B of
 * codes/engine.py:23,80 so no separate scaling pass is needed.
 * zero_batch_if_inf = 1 adds the training step's rule (_sanitize_loss, codes/engine.py:24-30): when
 * the batch loss is +-inf the reference replaces it by 0 * loss, so the WHOLE batch's gradient is
 * zero (the optimizer step still runs, on momentum alone); 0 = warp-ctc's per-utterance contract.
 *   acts (T,B,A); labels flat int32 (sum label_lens); label_offsets (B) int32 start of each
 *   utterance's labels; ws >= ds2_ctc_ws_bytes(T,B,A,max_label_len) bytes
 */
size_t ds2_ctc_ws_bytes(int T, int B, int A, int max_label_len);
int ds2_ctc_loss_grad(const float* acts, const int32_t* labels, const int32_t* label_offsets,
                      const int32_t* label_lens, const int32_t* act_lens, int T, int B, int A,
                      int max_label_len, float grad_scale, int zero_batch_if_inf, float* costs,
                      float* grad, void* ws, void* stream);

/* ------------------------------------------------------------------ MWER (csrc/ctc_mwer.hip)
 * Not in the reference.  Minimum-word-error-rate loss and gradient from N-best lists (Prabhavalkar et al. 2018; Shannon 2017):
 * utterance b owns the label rows n = 0 .. hyp_count[b] - 1 of hyp (B,N,hyp_stride) with lengths hyp_len (B,N), as
 * ds2_ctc_beam_search_nbest writes them, a risk W_n = risk[b][n] per row (its word or character distance to the reference,
 * ds2_edit_stats), and a reference given as for ds2_ctc_loss_grad.  acts (T,B,A) un-normalised, blank 0.  With
 *   c_n   = -log P(y_n | acts[:act_lens[b], b]), the EXACT CTC cost of row n by forward-backward (not the search's pruned
 *           ctc_logp), c_ref the reference's,
 *   P_n   = exp(-c_n) / sum_m exp(-c_m)   over the rows of finite cost, in float64,
 *   E_b   = sum_n P_n W_n                 the expected risk,
 *   loss_b = E_b + ctc_weight * c_ref     (left to the caller: exp_risk and ref_costs are outputs),
 *   grad  = grad_scale * sum_b ( sum_n w_n * dc_n/dacts + ctc_weight * dc_ref/dacts ),   w_n = -P_n (W_n - E_b),
 * where dc/dacts = softmax - occupancy as in ds2_ctc_loss_grad.  The rules:
 *   - a row of infinite cost has P = 0 and no gradient; its risk is not read;
 *   - a row longer than max_label_len (or than hyp_stride, or of negative length) is dropped: it counts as a row of infinite
 *     cost and dropped[b] counts it;
 *   - an utterance with no finite row has E = 0 and only its CTC term;
 *   - an utterance whose reference is infeasible (or longer than max_label_len) has ref_costs = +inf and contributes no gradient
 *     at all, neither term; its exp_risk is still reported;
 *   - zero_batch_if_inf = 1 applies the training step's rule of ds2_ctc_loss_grad: a reference of infinite cost zeroes the whole
 *     batch's gradient;
 *   - rows at or past hyp_count[b] are never read (labels, lengths and risks there may hold anything); their hyp_costs is +inf
 *     and their posterior 0;
 *   - frames at or past act_lens[b] get zero gradient, and what acts holds there (NaN included) is harmless;
 *   - adding a constant to every W_n of an utterance leaves the gradient unchanged up to rounding (sum_n w_n = 0).
 * Risks are expected within +-2^15 (they are label counts); the weighted occupancies are summed in 64-bit fixed point of 2^-44
 * units, so the result is bit-identical from run to run and does not depend on what ws held.
 * Outputs: ref_costs (B), hyp_costs (B,N), posterior (B,N) = P_n, exp_risk (B) = E_b, dropped (B), grad (T,B,A).
 * 1 <= N <= DS2_MWER_MAX_NBEST; max_label_len <= 511 and A <= 256 as for ds2_ctc_loss_grad; ctc_weight >= 0;
 * ws >= ds2_ctc_mwer_ws_bytes(T,B,A,N,max_label_len) bytes = two fp64 planes of (B (N+1), T, 2 max_label_len + 1) and small
 * change; the query returns 0 for sizes the entry refuses.  DS2_ERR_ARG before any launch for a NULL pointer or a size outside
 * these ranges.  Four launches on the stream (row log-sum-exp once per frame, one alpha / beta recursion per row and direction,
 * the weights per utterance, the gradient per frame); no global atomics, and neither acts nor the gradient is replicated per row.
 * Added without a change of DS2_ABI_VERSION: two new symbols, no existing signature altered. */
#define DS2_MWER_MAX_NBEST 128
size_t ds2_ctc_mwer_ws_bytes(int T, int B, int A, int N, int max_label_len);
int ds2_ctc_mwer_grad(const float* acts, const int32_t* act_lens, int T, int B, int A, const int32_t* hyp,
                      const int32_t* hyp_len, const int32_t* hyp_count, int N, int hyp_stride, const float* risk,
                      const int32_t* ref, const int32_t* ref_offsets, const int32_t* ref_lens, int max_label_len,
                      float ctc_weight, float grad_scale, int zero_batch_if_inf, float* ref_costs, float* hyp_costs,
                      float* posterior, float* exp_risk, int32_t* dropped, float* grad, void* ws, void* stream);

/* ------------------------------------------------------------------ optimiser
 * clip_grad_norm_(params, max_norm) + SGD(momentum, nesterov) (codes/engine.py:87-90) over ONE
 * flat fp32 buffer of n elements (the model keeps params / grads / momentum flat).
 *   ds2_sumsq: partial sums of squares -> out[0] (double) ; ws >= ds2_sumsq_ws_bytes(n)
 *   ds2_clip_sgd_nesterov: coef = min(1, max_norm / (sqrt(sumsq[0] * norm_scale^2) + 1e-6)) is
 *   computed ON DEVICE from sumsq (no host sync); g' = g * grad_scale * coef;
 *   buf = first_step ? g' : momentum*buf + g'; p -= lr * (g' + momentum*buf)
 * grad_scale lets the data-parallel average (1/world) fold into the update.
 */
size_t ds2_sumsq_ws_bytes(size_t n);
int ds2_sumsq(const float* x, size_t n, double* out, void* ws, void* stream);
int ds2_clip_sgd_nesterov(float* p, const float* g, float* buf, size_t n, const double* sumsq,
                          float grad_scale, float max_norm, float lr, float momentum, int first_step,
                          void* stream);

/* Everything the host reads back after a training step (codes/engine.py:92-94: synchronize, loss.item()),
 * gathered by ONE launch into out[0..3] (double): sum_b costs[b]; sumsq[0] (the squared gradient norm, or 0
 * when sumsq is NULL); the OR of the n_err 32-bit words err_words[i] point at (device pointers held in a
 * device array; the persistent recurrence's sticky timeout flags); the number of +-inf costs. */
int ds2_step_stats(const float* costs, int B, const double* sumsq, const uint32_t* const* err_words, int n_err,
                   double* out, void* stream);

/* misc elementwise used by the layer glue */
int ds2_add2(const float* a, const float* b, size_t n, float* out, void* stream);

/* A HIP stream of the given priority (hipDeviceGetStreamPriorityRange: 1 = low, 0 = normal, -1 = high on
 * gfx950).  torch.cuda.Stream clamps priorities to [-1, 0], so the LOW-priority stream the weight-gradient GEMMs run
 * on (under the next layer's recurrence kernel, without taking CUs from the critical chain) is created here and
 * wrapped with torch.cuda.ExternalStream.  The caller owns the stream. */
int ds2_stream_create(int priority, void** stream_out);
int ds2_stream_destroy(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DS2HIP_H */
