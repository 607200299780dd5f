/*
 * ttsamd.h — C ABI of libttsamd.so: the MI355X (gfx950) FastPitch -> HiFi-GAN hot path.
 *
 * The reference (nipponjo/tts-arabic-pytorch) has no FFI/plugin interface; its boundary is
 * the Python class surface models.fastpitch.FastPitch2Wave / FastPitch.
 * Each entry point below replaces one reference *function* on that path and is what a
 * ctypes binding inside the reference's own modules would call (INTEGRATION.md shows the
 * stub).  Conventions:
 *   - plain C types only; every data pointer is a DEVICE pointer (tensor.data_ptr()) to
 *     contiguous row-major memory unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     0/NULL = the default stream.  Calls are asynchronous on that stream;
 *   - return 0 on success, a negative TTSAMD_E* code otherwise; ttsamd_last_error()
 *     returns a thread-local message;
 *   - no hidden device allocation on hot calls: the caller passes a workspace sized by the
 *     matching *_workspace_bytes query.  Handles are immutable after create, so concurrent
 *     calls with distinct workspaces/streams are allowed.
 */
#ifndef TTSAMD_H
#define TTSAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTSAMD_OK 0
#define TTSAMD_EINVAL (-1)   /* bad argument / shape / missing tensor */
#define TTSAMD_EHIP (-2)     /* HIP runtime error */
#define TTSAMD_ENOMEM (-3)   /* workspace too small / allocation failure */

/* One named host tensor of a checkpoint (fp32, row-major).  Names are the reference's
 * state_dict keys (models/fastpitch/networks.py:52-71; vocoder/__init__.py:15-16). */
typedef struct ttsamd_tensor {
    const char* name;
    const float* data;   /* host */
    int32_t ndim;
    int64_t shape[4];
} ttsamd_tensor;

/* pretrained/hifigan-asc-v1/config.json:2,11-15 */
typedef struct ttsamd_hifigan_cfg {
    int32_t num_mels;                 /* 80 */
    int32_t upsample_initial_channel; /* 512 */
    int32_t n_ups;                    /* 4 */
    int32_t upsample_rates[8];        /* 8,8,2,2 */
    int32_t upsample_kernel_sizes[8]; /* 16,16,4,4 */
    int32_t n_kernels;                /* 3 resblocks per stage */
    int32_t resblock_kernel_sizes[8]; /* 3,7,11 */
    int32_t n_dilations;              /* 3 */
    int32_t resblock_dilations[8][8]; /* (1,3,5) each */
    int32_t resblock;                 /* 1 = ResBlock1 (V1), 2 = ResBlock2 (V3: two convs per block, dilations [j][0] and [j][1];
                                       * n_dilations >= 2); 0 is read as 1, anything else is TTSAMD_EINVAL at create.  A ResBlock2
                                       * generator runs in exact fp32 only: under ttsamd_set_precision(1 | 2) its forward is TTSAMD_EINVAL */
} ttsamd_hifigan_cfg;

/* models/fastpitch/__init__.py:3-41 (net_config), only the fields inference reads */
typedef struct ttsamd_fastpitch_cfg {
    int32_t n_mel_channels;   /* 80 */
    int32_t n_symbols;        /* 148 */
    int32_t padding_idx;      /* 0 */
    int32_t d_model;          /* symbols_embedding_dim 384 */
    int32_t in_fft_n_layers, in_fft_n_heads, in_fft_d_head, in_fft_kernel, in_fft_filter;
    int32_t out_fft_n_layers, out_fft_n_heads, out_fft_d_head, out_fft_kernel, out_fft_filter;
    int32_t dur_kernel, dur_filter, dur_n_layers;
    int32_t pitch_kernel, pitch_filter, pitch_n_layers, pitch_emb_kernel;
    int32_t energy_conditioning, energy_kernel, energy_filter, energy_n_layers, energy_emb_kernel;
    int32_t n_speakers;
    float speaker_emb_weight;
} ttsamd_fastpitch_cfg;

/* models/tacotron2/tacotron2_ms.py:121-153 (Tacotron2MS.__init__ defaults), inference fields only */
typedef struct ttsamd_tacotron2_cfg {
    int32_t n_symbol;                       /* 40 */
    int32_t num_speakers;                   /* 1: no speaker embedding */
    int32_t speaker_embedding_dim;          /* 128 (used when num_speakers > 1) */
    int32_t symbol_embedding_dim;           /* 512 */
    int32_t encoder_embedding_dim;          /* 512 */
    int32_t encoder_n_convolution;          /* 3 */
    int32_t encoder_kernel_size;            /* 5 */
    int32_t n_mels;                         /* 80 */
    int32_t prenet_dim;                     /* 256 */
    int32_t attention_rnn_dim;              /* 1024 */
    int32_t decoder_rnn_dim;                /* 1024 */
    int32_t attention_hidden_dim;           /* 128 */
    int32_t attention_location_n_filter;    /* 32 */
    int32_t attention_location_kernel_size; /* 31 */
    int32_t postnet_n_convolution;          /* 5 */
    int32_t postnet_kernel_size;            /* 5 */
    int32_t postnet_embedding_dim;          /* 512 */
    float gate_threshold;                   /* 0.5 */
    int32_t decoder_early_stopping;         /* 1: stop once every utterance's gate fired; 0: always decode max_step frames
                                             *    (tacotron2_ms.py:139,169,197 -> torchaudio _Decoder.infer) */
} ttsamd_tacotron2_cfg;

/* models/diacritizers/shakkelha/network.py:10-27, shakkala/network.py:9-24 as one tagger geometry */
typedef struct ttsamd_tagger_cfg {
    int32_t n_vocab;          /* embedding rows (91 / 149) */
    int32_t emb_dim;          /* 25 / 288 */
    int32_t n_lstm;           /* bidirectional LSTM layers (2 / 3) */
    int32_t lstm_hidden[4];   /* per direction (256,256 / 288,144,96) */
    int32_t hard_sigmoid;     /* 1: gates i,f,o = clamp(0.2x+0.5,0,1) (shakkala/lstm_hsm.py:352-379) */
    int32_t bn_after_lstm0;   /* 1: eval BatchNorm1d between lstm0 and lstm1 (shakkala/network.py:35) */
    float bn_eps;
    int32_t n_dense;          /* Linear layers after the LSTMs, ReLU on all but the last (3 / 1) */
    int32_t dense_dim[4];     /* 512,512,19 / 28; the last one is the number of classes */
} ttsamd_tagger_cfg;

const char* ttsamd_last_error(void);
/* ABI revision of this header.  Bumped whenever a struct gains a field or an argument changes meaning (2: ttsamd_tacotron2_cfg
 * gained decoder_early_stopping, ttsamd_profile_read's third value became the number of timed sections; 3: ttsamd_dp_* may be
 * bound twice per process, one communicator per stream; 4: ttsamd_bfo_resblock_chain takes the kernel size as its last argument; 5: the ttsamd_bfo3_* entries, ttsamd_conv1d_ex; 6: ttsamd_set_option / ttsamd_get_option / ttsamd_option_name / ttsamd_options_check replace the per-call
 * environment reads, ttsamd_resblock_pair takes the size of `packed`, ttsamd_resblock_pair_packed_floats; 7: ttsamd_fastpitch_set_batch_mode;
 * 8: ttsamd_hifigan_cfg.resblock (ResBlock2 generators), ttsamd_resblock2 / ttsamd_resblock2_packed_floats).  ttsamd_version() returns the value the library was BUILT with: a caller
 * compiled against another revision must refuse to run (ttsamd/lib.py does). */
#define TTSAMD_ABI_VERSION 8
int32_t ttsamd_version(void);
/* Run-time routing options: every switch that routes between kernels / schedules that both ship (INTEGRATION.md lists them with their
 * defaults).  An option's value is seeded ONCE from the environment variable of the same name (TTSAMD_<NAME>) when the library is first
 * used and changed afterwards only here; `name` with or without the TTSAMD_ prefix, `value` as the variable would hold it (decimal, hex
 * for the masks), NULL or "" = unset (the default applies).  An unknown name or a value outside the option's range returns TTSAMD_EINVAL
 * and changes nothing.  ttsamd_get_option writes the current text ("" = unset); ttsamd_option_name(i) enumerates the names (NULL past the
 * last); ttsamd_options_check reports a malformed TTSAMD_<NAME> found in the environment at load (ttsamd/lib.py raises on it).  No
 * reference counterpart. */
int32_t ttsamd_set_option(const char* name, const char* value);
int32_t ttsamd_get_option(const char* name, char* value, int32_t capacity);
const char* ttsamd_option_name(int32_t index);
int32_t ttsamd_options_check(void);
/* 1 if a gfx950 device is visible to the HIP runtime, else 0 (never throws). */
int32_t ttsamd_device_ok(void);

/* ---- HiFi-GAN generator: replaces vocoder.load_hifigan + Generator.forward
 *      (vocoder/__init__.py:3-20, vocoder/hifigan/models.py:86-136) ------------------- */

/* Accepts weight-normalised checkpoints (`*.parametrizations.weight.original0/1`,
 * `*.weight_g/_v`) and folded ones (`*.weight`); folds w = g*v/||v|| (norm over all dims
 * but 0) on the host exactly as remove_weight_norm does (models.py:129-136). */
int32_t ttsamd_hifigan_create(const ttsamd_tensor* weights, int32_t n_weights,
                              const ttsamd_hifigan_cfg* cfg, void** handle);
int32_t ttsamd_hifigan_destroy(void* handle);
int64_t ttsamd_hifigan_workspace_bytes(void* handle, int32_t batch, int32_t t_max);
/* mel  [B][num_mels][t_max] (frames >= lens[b] are ignored), lens int64 [B] or NULL (all
 * t_max).  wave [B][hop*t_max]; samples >= hop*lens[b] are left untouched.  Every layer
 * zero-pads at the TRUE utterance edge, i.e. utterance b's result equals the reference's
 * unbatched Generator.forward(mel[b,:,:lens[b]]) (models/fastpitch/networks.py:340-341). */
int32_t ttsamd_hifigan_forward(void* handle, const float* mel, const int64_t* lens,
                               int32_t batch, int32_t t_max, float* wave,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* ---- FastPitch.infer split at its one data-dependent size (dec_lens):
 *      models/fastpitch/fastpitch/model.py:351-409 ------------------------------------ */

int32_t ttsamd_fastpitch_create(const ttsamd_tensor* weights, int32_t n_weights,
                                const ttsamd_fastpitch_cfg* cfg, void** handle);
int32_t ttsamd_fastpitch_destroy(void* handle);
int64_t ttsamd_fastpitch_encode_workspace_bytes(void* handle, int32_t batch, int32_t n_tokens);
int64_t ttsamd_fastpitch_decode_workspace_bytes(void* handle, int32_t batch, int32_t t_max);

/* Phase A (model.py:355-399 + the integer half of regulate_len :68-76).
 * ids int64 [B][L], zero-padded at the END of each row (text_collate_fn,
 * models/fastpitch/networks.py:16-35).  dur_tgt [B][L] / pitch_tgt [B][1][L] /
 * energy_tgt [B][1][L] may be NULL (use predictions).  pitch_mul/pitch_add apply the
 * reference's pitch_trf (networks.py:38-42) when != (1,0).
 * Outputs: enc_cond [B][d_model][L] (CHANNEL-FIRST conditioned encoder output, the input
 * of ttsamd_length_regulate), dur_pred [B][L], pitch_pred [B][1][L], energy_pred [B][L],
 * reps int64 [B][L] = (dur/pace+0.5).long(), dec_lens int64 [B].  The host reads
 * dec_lens (the reference syncs here too, model.py:76) to size phase B. */
int32_t ttsamd_fastpitch_encode(void* handle, const int64_t* ids, int32_t batch, int32_t n_tokens,
                                int32_t speaker, float pace, const float* dur_tgt,
                                const float* pitch_tgt, const float* energy_tgt,
                                float pitch_mul, float pitch_add, float max_duration,
                                float* enc_cond, float* dur_pred, float* pitch_pred,
                                float* energy_pred, int64_t* reps, int64_t* dec_lens,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* Float half of regulate_len (model.py:77-85) as a gather instead of the reference's
 * one-hot matmul: out[b][c][t] = enc[b][c][j] with cumsum[j] <= t < cumsum[j+1], zero for
 * t >= dec_len.  enc [B][C][L], reps int64 [B][L], out [B][C][t_max], idx int32 [B][t_max]
 * (token index per frame, -1 past the end) may be NULL.  Bit-exact indices. */
int32_t ttsamd_length_regulate(const float* enc, const int64_t* reps, int32_t batch,
                               int32_t n_tokens, int32_t channels, int32_t t_max,
                               float* out, int32_t* idx, void* stream);

/* Phase B (model.py:405-408): decoder FFT + proj.  x [B][d_model][t_max] channel-first
 * (output of ttsamd_length_regulate; clobbered), dec_lens int64 [B], mel [B][80][t_max].
 * t_max is the ROW WIDTH of x and mel and may exceed max(dec_lens): the length of the reference's padded batch is taken from
 * dec_lens (batches of 2 and more), the extra columns are padding.  Pass a multiple of 4 for batches: the Winograd and float4-epilogue
 * paths of the conv engine need 16-byte-aligned rows (ttsamd/engine.py: FastPitchEngine.infer rounds t_max up and returns a view). */
int32_t ttsamd_fastpitch_decode(void* handle, float* x, const int64_t* dec_lens, int32_t batch,
                                int32_t t_max, float* mel, void* workspace,
                                int64_t workspace_bytes, void* stream);

/* How a BATCH of utterances goes through ttsamd_fastpitch_encode / _decode of this handle (default 0; not a per-call argument: set it
 * between calls, not under a running one).
 *   0  the reference's padded-batch arithmetic: the hidden activations of the conv-FF blocks and of the predictors are not masked, so
 *      the last frames of an utterance depend on the longest one of its batch (FastPitch.infer on a padded batch,
 *      models/fastpitch/fastpitch/transformer.py:72-90, model.py:129-133) -- what tts(list, batch_size > 1) returns.
 *   1  every utterance as if it were alone in the call: those two convs read their input masked at the utterance's own length (every
 *      other op already masks), so row b equals FastPitch.infer(ids[b:b+1, :len_b]) -- the reference's batch_size = 1 loop
 *      (models/fastpitch/networks.py:402-411) as ONE ragged call.  Equal to the one-by-one calls within fp32 summation order.
 *      pitch_pred is 0 past a row's end in this mode -- a lone row's padding is zero -- where mode 0 holds pitch_add there, as the
 *      reference's padded batch does (the transform is applied to the masked prediction); the k = 3 pitch embedding reads that
 *      position at the row's last token. */
int32_t ttsamd_fastpitch_set_batch_mode(void* handle, int32_t mode);

/* ---- Mixed requests in one batch.  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.  The two calls above with
 *      per-row controls and a per-call batch mode; workspaces are those of ttsamd_fastpitch_encode_workspace_bytes /
 *      ttsamd_fastpitch_decode_workspace_bytes for the same batch and width.
 *   speaker_rows int32 [B], pace_rows / pitch_mul_rows / pitch_add_rows float [B]: DEVICE arrays, each may be NULL, in which case the
 *      scalar argument of the same name applies to every row (and is checked as the scalar entry checks it).  Row b is computed by the
 *      kernels of the scalar entries with row b's values in the scalars' place, the same expressions in the same order: its bits equal
 *      those of ttsamd_fastpitch_encode on the same ids with row b's values as scalars.
 *      Device values are trusted as `ids` are -- memory-safe, not reported: a speaker outside [0, n_speakers) is clamped into the table, a
 *      pace that is not > 0 is taken as 1.  Range errors are for the caller that has the values on the host (ttsamd/engine.py raises).
 *   flags: bit 0 = every row as if it were alone in the call (mode 1 above) for THIS call; the handle's mode is neither read nor written,
 *      so callers that share a handle cannot mix arithmetic.  Pass the same flags to both phases of a call.  Any other bit: TTSAMD_EINVAL. */
int32_t ttsamd_fastpitch_encode_rows(void* handle, const int64_t* ids, int32_t batch, int32_t n_tokens,
                                     int32_t speaker, float pace, const float* dur_tgt,
                                     const float* pitch_tgt, const float* energy_tgt,
                                     float pitch_mul, float pitch_add, float max_duration,
                                     float* enc_cond, float* dur_pred, float* pitch_pred,
                                     float* energy_pred, int64_t* reps, int64_t* dec_lens,
                                     void* workspace, int64_t workspace_bytes,
                                     const int32_t* speaker_rows, const float* pace_rows,
                                     const float* pitch_mul_rows, const float* pitch_add_rows,
                                     int32_t flags, void* stream);
int32_t ttsamd_fastpitch_decode_rows(void* handle, float* x, const int64_t* dec_lens, int32_t batch,
                                     int32_t t_max, float* mel, void* workspace,
                                     int64_t workspace_bytes, int32_t flags, void* stream);

/* ---- HiFi-GAN bias denoiser: replaces vocoder.hifigan.denoiser.Denoiser
 *      (vocoder/hifigan/denoiser.py:32-64 __init__, :66-72 forward).  STFT/ISTFT with
 *      n_fft = win = 1024, hop 256, periodic hann, center/reflect, onesided, unnormalised. --- */
int32_t ttsamd_denoiser_create(void** handle);
int32_t ttsamd_denoiser_destroy(void* handle);
int64_t ttsamd_denoiser_workspace_bytes(int32_t batch, int32_t n_max);
/* bias_spec[513] = |STFT(audio)|[:, frame 0]; audio [n] is the vocoder output for a zero mel
 * (denoiser.py:50-64); n_dev = device int64 holding n. */
int32_t ttsamd_denoiser_bias_spec(void* handle, const float* audio, const int64_t* n_dev, int32_t n,
                                  float* bias_spec, void* workspace, int64_t workspace_bytes,
                                  void* stream);
/* In place: wave[b][0 : 256*(nsamples[b]/256)] <- ISTFT(max(|X|-strength*bias,0) * e^{i arg X}).
 * wave [B][wave_stride], nsamples int64 [B] (device), every nsamples[b] > 512. */
int32_t ttsamd_denoise(void* handle, float* wave, int64_t wave_stride, const int64_t* nsamples,
                       int32_t batch, int32_t n_max, const float* bias_spec, float strength,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* The same with one strength per row (new symbol, no ABI bump): strength_rows float [B] on the device, not NULL.  A row whose strength
 * is > 0 gets the bits of ttsamd_denoise on the same batch with that scalar; any other row is left UNTOUCHED bit for bit (an STFT ->
 * ISTFT round trip is no identity in bits; the wrappers skip the call for denoise <= 0). */
int32_t ttsamd_denoise_rows(void* handle, float* wave, int64_t wave_stride, const int64_t* nsamples,
                            int32_t batch, int32_t n_max, const float* bias_spec, const float* strength_rows,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* ---- MelVocos('22k' / '24k') vocoder: replaces vocoder.vocos.pretrained.MelVocos
 *      (vocoder/vocos/pretrained.py:34-93; backbone models.py:26-89, ConvNeXtBlock modules.py:8-60,
 *      ISTFTHead heads.py:26-41, ISTFT "same" spectral_ops.py:33-75).  Weight names are the keys of
 *      MelVocos.state_dict() (backbone.*, head.out.*). ------------------------------------------- */
int32_t ttsamd_vocos_create(const ttsamd_tensor* weights, int32_t n_weights, int32_t input_channels,
                            int32_t dim, int32_t intermediate_dim, int32_t num_layers, void** handle);
int32_t ttsamd_vocos_destroy(void* handle);
int64_t ttsamd_vocos_workspace_bytes(void* handle, int32_t batch, int32_t t_max);
/* bias_vec[513] = clip(exp(log-magnitude of a zero mel [1,80,88]), max 100)[:, frame 0]
 * (make_denoising_vector, pretrained.py:59-71). */
int32_t ttsamd_vocos_bias_vec(void* handle, float* bias_vec, void* workspace, int64_t workspace_bytes,
                              void* stream);
/* mel [B][input_channels][t_max], lens int64 [B] (device) -> wave [B][256*t_max]; samples >= 256*lens[b] untouched.
 * mag = clamp(exp(.) - denoise*bias_vec, 0, 100) (pretrained.py:79-88). */
int32_t ttsamd_vocos_forward(void* handle, const float* mel, const int64_t* lens, int32_t batch,
                             int32_t t_max, float denoise, const float* bias_vec, float* wave,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* The same with one denoise strength per row (new symbol, no ABI bump): denoise_rows float [B] on the device, not NULL; bias_vec is
 * needed.  Row b gets the bits of ttsamd_vocos_forward on the same batch with denoise_rows[b] as the scalar (0: no subtraction). */
int32_t ttsamd_vocos_forward_rows(void* handle, const float* mel, const int64_t* lens, int32_t batch,
                                  int32_t t_max, const float* denoise_rows, const float* bias_vec, float* wave,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Added after ABI revision 8 WITHOUT a bump: ttsamd_vocos_set_padding and the ttsamd_melspec_* entries below are new symbols only;
 *      no existing signature, struct or argument meaning changed, so TTSAMD_ABI_VERSION stays 8.  A library built before them lacks the
 *      symbols, which a binding that lists them finds at load (ttsamd/lib.py resolves every name of its table; dlsym fails loudly). ----
 * ISTFT trimming of the Vocos head: 0 = "same" (the default; spectral_ops.py:47-75: 256 * lens[b] samples per utterance), 1 = "center"
 * (MelVocos('24k'); spectral_ops.py:44-46 = torch.istft(center=True): 256 * (lens[b] - 1) samples, none for one frame).  The wave rows keep
 * the stride 256 * t_max in both modes.  input_channels of ttsamd_vocos_create may be any positive count (100 for '24k'): the embed
 * conv's input channels are zero-padded to the engine's 8-channel chunks inside the library. */
int32_t ttsamd_vocos_set_padding(void* handle, int32_t mode);

/* ---- Mel analysis, wave -> (log-)mel, one launch: replaces utils.audio.MelSpectrogram.forward (utils/audio.py:35-46) and
 *      MelSpectrogramFeatures.forward (vocoder/vocos/feature_extractors.py:58-64).  n_fft = win = 1024 and hop_length = 256 only (anything
 *      else: TTSAMD_EINVAL), periodic hann, reflect padding at each utterance's own ends.
 *      fbank [n_mels][513] fp32 on the HOST, dense, copied at create (1 <= n_mels <= 128);
 *      framing 0 "same":   pad 384 per side, frames = n / 256      (needs n >= 385; utils.audio.MelSpectrogram, padding="same")
 *              1 "center": pad 512 per side, frames = n / 256 + 1  (needs n >= 513; torch.stft(center=True), padding="center");
 *      mag_mode 0: |X| (torchaudio power = 1), 1: sqrt(|X|^2 + 1e-9) (utils/audio.py:44);
 *      log_clip > 0: log(max(mel, log_clip)) (modules.py safe_log, 1e-5), <= 0: linear mel. ------------------------------------------- */
int32_t ttsamd_melspec_create(const float* fbank, int32_t n_mels, int32_t n_fft, int32_t hop_length, int32_t framing,
                              int32_t mag_mode, float log_clip, void** handle);
int32_t ttsamd_melspec_destroy(void* handle);
/* wave [B][wave_stride], nsamples int64 [B] (device) -> mel [B][n_mels][t_max] (device), row b = the call on wave[b][0 : nsamples[b]]
 * alone, bit for bit; frames at or past the row's own count are written as zero.  frames_out int64 [B] (device, may be NULL) receives
 * min(frame count of the table above, t_max): the `lens` of the vocoder call that follows, no host synchronisation in between.
 * A row shorter than the framing needs gives values but no meaning (indices are kept inside the row; the Python wrappers raise). */
int32_t ttsamd_melspec_forward(void* handle, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch,
                               int32_t t_max, float* mel, int64_t* frames_out, void* stream);

/* ---- Oversmoothing analysis (utils/oversmoothing.py, utils/metrics.py of the reference; csrc/oversmooth.hip).  Like the ttsamd_melspec_*
 *      entries these are new symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.  Every pointer is device memory, lengths are
 *      int64 [batch]; a length is clamped to [0, t_max].  No call reads anything back to the host.
 *      The longest series ttsamd_series_summary sorts and the longest side ttsamd_dtw aligns: */
#define TTSAMD_OVERSMOOTH_MAX_FRAMES 4096
/* mel [B][n_mels][t_max] -> series [B][4][t_max] fp32: per frame, from the power of an rFFT across the bands (Q = n_mels / 2 + 1 bins):
 *   0 HQER      hqer_scale * sum P[q_c .. Q-1] / (sum P[1 .. Q-1] + 1e-12)   (q_c = -1: clamp(floor(0.25 Q), 1, Q - 1); the drop-in scales by 100)
 *   1 CSlope    least-squares slope of 10 log10(P + 1e-8) over q = 1 .. Q-1 (NaN for fewer than two points)
 *   2 CCentroid sum q P / (sum P + 1e-12) over q >= 1
 *   3 CRoll95   first q whose cumulative power from q = 1 reaches 0.95 (total + 1e-12), 1 if none does
 * center != 0 subtracts the frame's mean over the bands, hann != 0 applies np.hanning(n_mels) (symmetric, rounded once to fp32).
 * 1 <= n_mels <= 128.  Intermediate arithmetic is float64.  Frames at or past lens[b] are written as zero; row b equals the call on
 * row b alone, bit for bit.  `power` (may be NULL) receives P itself, [B][Q][t_max] fp32 (framewise_rfft_power). */
int32_t ttsamd_cepstral_series(const float* mel, const int64_t* lens, int32_t batch, int32_t n_mels, int32_t t_max, int32_t center,
                               int32_t hann, int32_t q_c, float hqer_scale, float* power, float* series, void* stream);
/* The same four series from a power [B][n_q][t_max] the caller holds (hqer_from_power, slope_from_power, ... of the reference), with
 * their parameters: the slope over q1 .. q2 (0 <= q1, q2 <= n_q - 1; NaN for fewer than two points) of 10 log10(P + eps), the roll-off
 * at the fraction roll_p.  1 <= n_q <= 65. */
int32_t ttsamd_cepstral_series_from_power(const float* power, const int64_t* lens, int32_t batch, int32_t n_q, int32_t t_max, int32_t q_c,
                                          int32_t q1, int32_t q2, double eps, double roll_p, float hqer_scale, float* series,
                                          void* stream);
/* series [B][n_series][t_max], lens [B] (one length for the n_series series of a row) ->
 *   stats [B][n_series][3]: count, mean and median of the finite values (NaN, NaN for none; the median of an even count is the mean of
 *                           the two middle values);
 *   feat  [B][n_series][t_max]: the copy DTW aligns: NaNs interpolated linearly between their finite neighbours (the ends clamp; all-NaN
 *                           gives zeros), then (x - m) / s in fp32 with the mean m and the population standard deviation s computed in
 *                           float64 and rounded to fp32; zeros when s is 0 or not finite, and past lens[b].
 * t_max <= TTSAMD_OVERSMOOTH_MAX_FRAMES, else TTSAMD_EINVAL. */
int32_t ttsamd_series_summary(const float* series, const int64_t* lens, int32_t batch, int32_t n_series, int32_t t_max, float* stats,
                              float* feat, void* stream);
/* DTW of a [B][channels][ta_max] against b [B][channels][tb_max] (channels = 1: plain series): metric 0 = L2, 1 = cosine; window -1 = no
 * band, >= 0 the Sakoe-Chiba radius.  cost [B] fp32 = D[Ta][Tb]; path int32 [B][ta_max + tb_max][2] = (i, j) in ascending time, zeros past
 * path_len [B] (int32).  All arithmetic is single fp32 operations in the reference's order (local cost summed over the channels in order,
 * D = cost + best, unwritten cells read 1e30f, predecessor by strict < in the order up, left, diag), so path and cost are reproducible bit
 * for bit, in a batch or alone.  A band narrower than |Ta - Tb| gives path_len 0 and cost 1e30f; an empty side gives path_len 0 and cost
 * 1e30f (0 when both are empty).  ta_max, tb_max <= TTSAMD_OVERSMOOTH_MAX_FRAMES.  `workspace` (4-byte aligned) holds the backpointers,
 * two bits per cell of the diagonal-major table: ttsamd_dtw_workspace_bytes() bytes (-1 for arguments ttsamd_dtw refuses); a smaller
 * buffer is TTSAMD_EINVAL and nothing is launched. */
int64_t ttsamd_dtw_workspace_bytes(int32_t batch, int32_t ta_max, int32_t tb_max, int32_t channels);
int32_t ttsamd_dtw(const float* a, const int64_t* lens_a, const float* b, const int64_t* lens_b, int32_t batch, int32_t channels,
                   int32_t ta_max, int32_t tb_max, int32_t metric, int32_t window, float* cost, int32_t* path, int32_t* path_len,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* mae [B] = mean over k < path_len[b] of |pred[b][path[b][k][0]] - ref[b][path[b][k][1]]| (pred [B][ta_max], ref [B][tb_max]; differences in
 * fp32, the sum in float64; NaN for an empty path). */
int32_t ttsamd_dtw_aligned_mae(const float* pred, const float* ref, int32_t batch, int32_t ta_max, int32_t tb_max, const int32_t* path,
                               const int32_t* path_len, float* mae, void* stream);

/* ---- Objective evaluation of a prediction against a recording (csrc/objective.hip): mel-cepstral distortion, mel error, F0 errors and
 *      voicing error along a path of ttsamd_dtw.  The reference has no such module: the arithmetic below is the specification.  New
 *      symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.  Every pointer is device memory, lengths are int64 [batch], read
 *      on the device and clamped to the padded size.  No call reads anything back to the host. */
/* logmel [B][n_mels][t_max] fp32 -> cep [B][n_coef][t_max] fp32: the orthonormal DCT-II across the bands of every frame,
 *   c_k[t] = s_k sum_{m < M} x_m[t] cos(pi k (2m + 1) / (2M)),  s_0 = sqrt(1 / M), s_k = sqrt(2 / M)
 * (scipy.fft.dct(x, type=2, norm='ortho', axis=bands)[:n_coef]).  Products and sums are float64 over m ascending, the basis comes from a
 * float64 table with the argument reduced mod 4M in integers; the result is rounded once to fp32.  1 <= n_mels <= 128,
 * 1 <= n_coef <= min(n_mels, 64), else TTSAMD_EINVAL.  Frames at or past lens[b] are written as zero and never read; row b equals the
 * call on row b alone, bit for bit. */
int32_t ttsamd_mel_cepstrum(const float* logmel, const int64_t* lens, int32_t batch, int32_t n_mels, int32_t t_max, int32_t n_coef, float* cep,
                            void* stream);
/* The scores of pair b along its path: cep_a [B][n_coef][ta_max], cep_b [B][n_coef][tb_max]; mel_a / mel_b [B][n_mels][t*_max] (both may
 * be NULL); f0_a / f0_b [B][t*_max] in Hz (both may be NULL); path int32 [B][ta_max + tb_max][2] and path_len int32 [B] exactly as
 * ttsamd_dtw writes them (steps (i_p, j_p), p < n = path_len[b]; indices are clamped to the padded size).  A frame is voiced when its f0
 * is finite and > 0.  stats [B][TTSAMD_EVAL_STATS] FLOAT64:
 *   0 n              path_len[b]
 *   1 mcd            scale mean_p sqrt(sum_{c = first_coef}^{n_coef - 1} (cep_a[c][i_p] - cep_b[c][j_p])^2)   (10 sqrt(2) / ln 10 gives dB;
 *                    first_coef = 1 leaves c0, the level, out)
 *   2 mel_mae        mean over p and m of |mel_a[m][i_p] - mel_b[m][j_p]|; NaN without mels
 *   3 n_vv           steps where both frames are voiced
 *   4 f0_rmse_cents  sqrt(mean over those steps of (1200 log2(f0_a / f0_b))^2)
 *   5 f0_rmse_hz     sqrt(mean over those steps of (f0_a - f0_b)^2)
 *   6 f0_corr        Pearson correlation of the two f0 over those steps, in two passes (the means, then the centred sums); NaN when
 *                    n_vv < 2 or a centred sum of squares is 0
 *   7 vuv_error      (steps whose two frames differ in voicing) / n
 * Every input is widened to float64 before the first subtraction.  n = 0: n = 0, n_vv = 0, NaN elsewhere; n_vv = 0: NaN in 4..6; without
 * f0: NaN in 3..7.  first_coef outside [0, n_coef) is TTSAMD_EINVAL.  One block per pair; step p is added by thread p mod 256 in
 * ascending order and the block sum is a fixed tree, so row b equals the call on pair b alone, bit for bit. */
#define TTSAMD_EVAL_STATS 8
int32_t ttsamd_dtw_aligned_eval(const float* cep_a, const float* cep_b, int32_t n_coef, int32_t first_coef, const float* mel_a,
                                const float* mel_b, int32_t n_mels, const float* f0_a, const float* f0_b, int32_t batch, int32_t ta_max,
                                int32_t tb_max, const int32_t* path, const int32_t* path_len, double scale, double* stats, void* stream);

/* ---- FastPitch forced alignment (the aligner path of FastPitch.forward, models/fastpitch/fastpitch/model.py:298-318,331-332: ConvAttention,
 *      binarize_attention with mas_width1, average_pitch; csrc/aligner.hip).  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays
 *      8.  Every pointer is device memory, lengths are int64 [batch] and are clamped to the padded size.  No call reads anything back to the
 *      host.  ttsamd_set_precision does not reach these entries: the encoders' hidden layers are fp32 MFMA, their last 1 x 1 conv and the
 *      squared distances accumulate in float64, the softmax and MAS are fp32.  The most tokens per row ttsamd_mas and ttsamd_aligner_forward take: */
#define TTSAMD_MAS_MAX_TOKENS 1024
typedef struct ttsamd_aligner_cfg {
    int32_t n_mel;        /* 80: query channels (a multiple of 8) */
    int32_t d_text;       /* 384: symbols_embedding_dim, the key channels (a multiple of 16) */
    int32_t n_att;        /* 80: channels both encoders end in (<= 96) */
    int32_t n_symbols;    /* rows of encoder.word_emb.weight */
    int32_t padding_idx;  /* its row is loaded as given (zero in the reference's checkpoints) */
} ttsamd_aligner_cfg;
/* Weights by their names in FastPitch.state_dict(): encoder.word_emb.weight, attention.key_proj.{0,2}.conv.{weight,bias},
 * attention.query_proj.{0,2,4}.conv.{weight,bias}.  attention.attn_proj.* is unused by the reference's forward and ignored; a missing
 * tensor is TTSAMD_EINVAL naming it. */
int32_t ttsamd_aligner_create(const ttsamd_tensor* weights, int32_t n_weights, const ttsamd_aligner_cfg* cfg, void** handle);
int32_t ttsamd_aligner_destroy(void* handle);
int64_t ttsamd_aligner_workspace_bytes(void* handle, int32_t batch, int32_t n_tokens, int32_t n_frames);
/* ConvAttention.forward (attention.py:174-223): ids int64 [B][n_tokens], mel [B][n_mel][n_frames], attn_prior [B][n_frames][n_tokens] or
 * NULL -> attn_soft, attn_logprob [B][n_frames][n_tokens] fp32.  Both encoders run over the padded batch without masks, as the reference
 * runs them: frames and tokens past a row's length are read as the caller passed them.  logit = -0.0005 sum_c (q - k)^2, summed directly;
 * with a prior, log_softmax over all n_tokens + log(prior + 1e-8); attn_logprob is that value before masking; tokens >= in_lens[b] are
 * then masked (attn_soft exactly 0 there) and attn_soft is the softmax over the rest.  Frames >= mel_lens[b] are computed like the others
 * (mel_lens may be NULL: the reference's attention never reads it).  n_tokens <= TTSAMD_MAS_MAX_TOKENS. */
int32_t ttsamd_aligner_forward(void* handle, const int64_t* ids, const int64_t* in_lens, const float* mel, const int64_t* mel_lens,
                               const float* attn_prior, int32_t batch, int32_t n_tokens, int32_t n_frames, float* attn_soft,
                               float* attn_logprob, void* workspace, int64_t workspace_bytes, void* stream);
/* Monotonic alignment search, mas_width1 of alignment.py:46-72 bit for bit, on row b's [:out_lens[b], :in_lens[b]] corner of attn
 * [B][n_frames][n_tokens]: is_log != 0: attn holds the log-attention; 0: attn holds probabilities and logf of the stored fp32 value is
 * taken first (model.py:248).  log_p[0][1:] = -inf; log_p[i][j] += max(log_p[i-1][j-1], log_p[i-1][j]) as one fp32 max and one fp32 add;
 * the backtrack moves to j - 1 when log_p[i-1][j-1] >= log_p[i-1][j] (ties, two -inf among them, go to j - 1) and stays at token 0 once it
 * is there.  n_frames < n_tokens follows the same rule.  in_lens[b] == 1: the reference indexes out of bounds there; defined as every
 * frame assigned to token 0.  dur [B][n_tokens] fp32 = frames per token (zero past in_lens[b]; all zero when out_lens[b] or in_lens[b] is
 * 0); attn_hard [B][n_frames][n_tokens] (may be NULL) = the 0 / 1 path, zero outside the corner.  `workspace` (8-byte aligned) holds the
 * decisions at one bit per cell when they do not fit in LDS: ttsamd_mas_workspace_bytes() bytes (often 0; -1 for arguments ttsamd_mas
 * refuses).  n_tokens > TTSAMD_MAS_MAX_TOKENS is TTSAMD_EINVAL. */
int64_t ttsamd_mas_workspace_bytes(int32_t batch, int32_t n_frames, int32_t n_tokens);
int32_t ttsamd_mas(const float* attn, int32_t is_log, const int64_t* in_lens, const int64_t* out_lens, int32_t batch, int32_t n_frames,
                   int32_t n_tokens, float* dur, float* attn_hard, void* workspace, int64_t workspace_bytes, void* stream);
/* average_pitch (model.py:93-111): pitch [B][n_formants][n_frames], dur [B][n_tokens] -> out [B][n_formants][n_tokens]: per token the mean
 * of the non-zero values among its frames [e[l-1], e[l]), e = cumsum(dur) in fp32 truncated to an integer as the reference takes it
 * (clamped to n_frames); 0 where no frame of the segment is non-zero.  Each segment is summed directly (float64, rounded once). */
int32_t ttsamd_average_pitch(const float* pitch, const float* dur, int32_t batch, int32_t n_formants, int32_t n_frames, int32_t n_tokens,
                             float* out, void* stream);

/* ---- The alignment prior and the alignment scores of the reference's aligner training, forward only (BetaBinomialInterpolator and
 *      beta_binomial_prior_distribution of fastpitch/data_function.py:45-78; AttentionCTCLoss and AttentionBinarizationLoss of
 *      fastpitch/attn_loss_function.py; csrc/attn_loss.hip).  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.  Every
 *      pointer is device memory (ttsamd_attn_prior_tables: host), lengths are int64 [batch] and are clamped to the padded size.  No call
 *      reads anything back to the host.  ttsamd_set_precision does not reach these entries: everything is float64 up to the stored value.
 *      No gradient is built.
 *
 * The prior of row b: its [mel_lens[b], in_lens[b]] corner of out [B][n_frames][n_tokens] fp32, ZERO outside it (as TTSCollate pads).
 *   mode 0, exact: out[i-1][k] = betabinom(n = P, a = scaling i, b = scaling (M + 1 - i)).pmf(k), k = 0 .. P - 1, with P = in_lens[b] and
 *     M = mel_lens[b] (n = P, not P - 1: a row does not add up to 1; the reference's behaviour, kept).
 *   mode 1, interpolated: what BetaBinomialInterpolator()(w = mel_len, h = in_len) returns, the prior the checkpoints were trained with:
 *     bw = max(1, rint((w + 1) / 100)) 100 and bh = max(1, rint((h + 1) / 20)) 20 (halves to even, as np.round), the bank
 *     beta_binomial_prior_distribution(phoneme_count = bw, mel_count = bh) transposed (the reference passes the rounded MEL length as the
 *     phoneme count; reproduced), sampled as scipy.ndimage.zoom(bank, (w / bw, h / bh), order=1) does: cell (o, p) at x = o (bw - 1) /
 *     (w - 1), y = p (bh - 1) / (h - 1) (0 when the extent is 1), bilinear between floor and floor + 1 clamped to the last index, float64.
 *   mode | TTSAMD_ATTN_PRIOR_F64: out is float64 [B][n_frames][n_tokens] (the values before the rounding to fp32).
 * Only scaling == 1.0 is built (anything else: TTSAMD_EINVAL): with integer a, b the pmf is exp of nine entries of lf[n] = log n!, a table
 * built once per device on the host in float64 (std::lgamma) and uploaded at the first call that needs it.  ttsamd_attn_prior_tables
 * writes lf[0 .. n) to HOST memory: the table, for checking it without a device. */
#define TTSAMD_ATTN_PRIOR_F64 2
int32_t ttsamd_attn_prior(const int64_t* in_lens, const int64_t* mel_lens, int32_t batch, int32_t n_tokens, int32_t n_frames, int32_t mode,
                          double scaling, void* out, void* stream);
int32_t ttsamd_attn_prior_tables(int32_t n, double* lf);
/* Forward-sum loss per row: nll [B] float64 = the CTC negative log-likelihood of the targets 0 .. in_lens[b] - 1 (in order, blanks between)
 * over the frames t < out_lens[b], frame t's distribution being [blank_logprob, attn_logprob[b][t][:in_lens[b]]] log-softmaxed (tokens past
 * in_lens[b] masked).  attn_logprob [B][n_frames][n_tokens] fp32; all arithmetic is float64 in the log domain.  out_lens[b] < in_lens[b] (no
 * path; also 0 frames for some tokens): +inf.  in_lens[b] == 0: 0.  AttentionCTCLoss's scalar is the mean over rows of (nll, 0 where
 * infinite) / max(in_lens, 1).  Two launches whatever the length: the per-frame normalisers into `workspace` (8-byte aligned,
 * ttsamd_attn_ctc_loss_workspace_bytes() bytes; -1 for arguments the call refuses), then one block per row.  n_tokens >
 * TTSAMD_MAS_MAX_TOKENS is TTSAMD_EINVAL. */
int64_t ttsamd_attn_ctc_loss_workspace_bytes(int32_t batch, int32_t n_frames, int32_t n_tokens);
int32_t ttsamd_attn_ctc_loss(const float* attn_logprob, const int64_t* in_lens, const int64_t* out_lens, int32_t batch, int32_t n_frames,
                             int32_t n_tokens, double blank_logprob, double* nll, void* workspace, int64_t workspace_bytes, void* stream);
/* Binarization loss per row: sum_log [B] = the sum of log(max(attn_soft, eps)) over the cells with attn_hard == 1, count [B] = how many
 * there are; attn_hard, attn_soft [B][n_frames][n_tokens] fp32, the sums float64 in a fixed order (the same bits run to run).
 * AttentionBinarizationLoss's scalar is -sum(sum_log) / sum(count). */
int32_t ttsamd_attn_bin_loss(const float* attn_hard, const float* attn_soft, int32_t batch, int32_t n_frames, int32_t n_tokens, double eps,
                             double* sum_log, double* count, void* stream);

/* ---- pYIN pitch tracking, wave -> (f0, voiced_flag, voiced_prob) per frame (librosa.pyin as the reference calls it in
 *      scripts/extract_f0.py:34-39 and fastpitch/data_function.py:81-114; csrc/pyin.hip).  New symbols only, added WITHOUT a bump:
 *      TTSAMD_ABI_VERSION stays 8.  Two launches per call whatever the length: a frame kernel (difference function, cumulative-mean
 *      normalisation, troughs, threshold distribution, pitch bins; one block per frame) and a Viterbi kernel (one block per row, the
 *      time loop and the backtrack inside).  The arithmetic (DESIGN.md section 4 states it in full):
 *        W = win_length, pmin = max(floor(sr / fmax), 1), pmax = min(ceil(sr / fmin), frame_length - W - 1), nb = ceil(1 / resolution),
 *        P = floor(12 nb log2(fmax / fmin)) + 1 pitch bins, tiny = the smallest normal double;
 *        the row is padded by frame_length / 2 per side, frame t = padded[t hop, t hop + frame_length), frames = 1 + n / hop;
 *        d(tau) = sum_{j < W} (x[j] - x[j + tau])^2, summed DIRECTLY in float64 over j ascending (the reference's FFT route and its
 *        clamp of values below 1e-6 are deliberately not reproduced), d'(tau) = d(tau) / (cumsum(d)(tau) / tau + tiny);
 *        troughs of d' over tau = pmin..pmax with parabolic refinement; thresholds k / n_thresholds weighted by the Beta(beta_a, beta_b)
 *        CDF in closed form; Boltzmann prior over the troughs under each threshold; the lowest trough gains no_trough_prob times the
 *        weight of the thresholds it is not under; candidates go to bins of 1 / nb semitone above fmin (two troughs in a bin: the
 *        larger lag wins); a 2 P-state HMM (voiced bins, then unvoiced) with a triangular local transition of width
 *        w = round(max_transition_rate 12 hop / sr) nb + 1 (cut at the ends, rows normalised) times the switch matrix, uniform start;
 *        Viterbi in fp32 over tables computed in float64 and rounded, every log as log(x + tiny), ties to the LOWEST state index.
 *      Byte parity with a particular librosa release is not pinned.
 *      Limits (TTSAMD_EINVAL at create): frame_length even and <= 2048, 1 <= win_length < frame_length, P <= 1024, n_thresholds <= 128,
 *      beta_a and beta_b positive integers (<= 64), w odd with min(P, w) * w <= 12288 table entries, at least three lags. */
#define TTSAMD_PYIN_MAX_FRAMES 8192   /* 95 s at hop 256 / 22050 Hz; the workspace of one such row at the defaults: 27.9 MB */
typedef struct ttsamd_pyin_cfg {
    int32_t sample_rate;          /* 22050 */
    int32_t frame_length;         /* 1024 in the reference's two calls (librosa's default: 2048) */
    int32_t win_length;           /* frame_length / 2 */
    int32_t hop_length;           /* 256 (librosa's default: frame_length / 4) */
    double fmin, fmax;            /* C2 = 65.406..., C7 = 2093.004... */
    int32_t n_thresholds;         /* 100 */
    int32_t beta_a, beta_b;       /* 2, 18 */
    double boltzmann;             /* 2 */
    double resolution;            /* 0.1 */
    double max_transition_rate;   /* 35.92 octaves per second */
    double switch_prob;           /* 0.01 */
    double no_trough_prob;        /* 0.01 */
    int32_t pad_mode;             /* 0 constant (zeros), 1 reflect (periodic reflection about the row's own ends) */
} ttsamd_pyin_cfg;
/* The tables the kernels read, computed on the HOST in float64 from cfg alone (no device is touched; create uploads the same ones).
 * dims [8] = pmin, pmax, P, nb, w, E (the most observations a frame can hold, (pmax - pmin + 2) / 2), n_kinds = min(P, w) distinct
 * transition rows, 0.  Any table pointer may be NULL: beta [n_thresholds]; expn [E + 1] = exp(-boltzmann p); norm [E + 1] =
 * (1 - exp(-boltzmann)) / (1 - exp(-boltzmann N)), norm[0] = 0: the prior of position p among N troughs is expn[p] * norm[N];
 * trans [n_kinds][w][2] = probability of (source row kind, column d = destination - source + w / 2) without / with a voiced-unvoiced
 * switch, 0 where the destination is cut off; logtrans fp32 [n_kinds][w][2] = log(trans + tiny) rounded; f0 fp32 [P].
 * Row kind of source bin k: k when P <= w; else k for k < w / 2, k - (P - w) for k >= P - w / 2, w / 2 for every interior row. */
int32_t ttsamd_pyin_tables(const ttsamd_pyin_cfg* cfg, int32_t* dims, double* beta, double* expn, double* norm, double* trans,
                           float* logtrans, float* f0);
int32_t ttsamd_pyin_create(const ttsamd_pyin_cfg* cfg, void** handle);
int32_t ttsamd_pyin_destroy(void* handle);
/* Bytes of `workspace` for a call of `batch` rows and t_max = n_frames: the sparse observations (per frame a count, the unvoiced
 * log-probability and up to E (fp32 log-probability, uint16 bin) pairs) and the Viterbi back-pointers (uint16 [batch][n_frames][2 P]).
 * -1 for arguments ttsamd_pyin_forward refuses (NULL handle, batch < 1, n_frames < 1 or > TTSAMD_PYIN_MAX_FRAMES). */
int64_t ttsamd_pyin_workspace_bytes(void* handle, int32_t batch, int32_t n_frames);
/* wave [B][wave_stride] fp32, nsamples int64 [B] (clamped to [0, wave_stride]) -> f0 [B][t_max] fp32 (Hz; 0 on unvoiced frames),
 * voiced_flag uint8 [B][t_max], voiced_prob [B][t_max] FLOAT64 (as computed: a sum of table values), states int32 [B][t_max] (may be NULL: the Viterbi state, < P voiced bin,
 * >= P unvoiced; -1 past the row), frames_out int64 [B] (may be NULL) = min(1 + nsamples[b] / hop, t_max).  Every pointer is device
 * memory (256-byte aligned workspace), nothing is read back to the host.  Row b equals the call on wave[b][0 : nsamples[b]] alone, bit for
 * bit; frames at or past a row's count are written as f0 = 0, flag = 0, prob = 0.  The workspace keeps the observations after the call
 * at the byte offsets ttsamd_pyin_obs_offsets writes to obs_offsets int64 [4] (host): counts int32 [B][t_max], unvoiced fp32 [B][t_max],
 * log-probabilities fp32 [B][t_max][E], bins uint16 [B][t_max][E] (descending within a frame; only the first count entries are written). */
int32_t ttsamd_pyin_forward(void* handle, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t t_max,
                            float* f0, uint8_t* voiced_flag, double* voiced_prob, int32_t* states, int64_t* frames_out,
                            void* workspace, int64_t workspace_bytes, void* stream);
int32_t ttsamd_pyin_obs_offsets(void* handle, int32_t batch, int32_t n_frames, int64_t* obs_offsets);

/* ---- Recording preparation: polyphase sinc resampling (torchaudio.functional.resample, 'sinc_interp_hann', as the reference calls it in
 *      scripts/preprocess_audio.py:33-47 and utils/data.py:59-67; csrc/resample.hip), silence trimming with peak normalisation
 *      (librosa.effects.trim with ref = np.max and numpy's x / max|x| * 0.999) and removal of silent mel frames (utils/data.py
 *      remove_silence; csrc/trim.hip).  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.  Every pointer is device memory
 *      unless it says host, lengths are read on the device, nothing is read back to the host.
 *      Resampler arithmetic (the table is built by the caller: ttsamd/resample.py): g = gcd(orig, new), o = orig / g, n = new / g,
 *        base = min(o, n) rolloff, width = ceil(lowpass_filter_width o / base), J = 2 width + o; for j < J, p < n in float64:
 *        t = clamp(((j - width) / o - p / n) base, -lfw, +lfw), taps[p][j] = sinc(t) cos^2(t pi / lfw / 2) base / o, rounded once to fp32;
 *        out[f n + p] = sum_{j < J} taps[p][j] xz[f o + j - width], xz = the row, zero outside it, summed over j ascending as one fp32 fma
 *        chain (both kernels); a row of L samples has ceil(n L / o) outputs.  Parity with a torchaudio release is not pinned.
 *      Limits (TTSAMD_EINVAL at create): 1 <= o, n <= 4096, J <= 65536. */
/* taps: HOST [n][J] fp32.  The handle keeps the table on the device, transposed and zero-padded to the kernels' tiles. */
int32_t ttsamd_resample_create(const float* taps, int32_t o, int32_t n, int32_t width, void** handle);
int32_t ttsamd_resample_destroy(void* handle);
/* host helper: ceil(n nsamples / o) in int64 (0 for nsamples <= 0; -1 for a NULL handle) */
int64_t ttsamd_resample_out_len(void* handle, int64_t nsamples);
/* 1 when route 2 of ttsamd_resample_forward accepts this handle, else 0 */
int32_t ttsamd_resample_mfma_eligible(void* handle);
/* wave [B][wave_stride] fp32, nsamples int64 [B] (clamped to [0, wave_stride]) -> out [B][out_stride] fp32, nout int64 [B] (may be NULL)
 * = ceil(n nsamples[b] / o).  Row b equals the call on wave[b][0 : nsamples[b]] alone, bit for bit (and both routes run the same fma chain);
 * samples of out at or past nout[b], up to out_stride, are written as zero; nothing at or past nsamples[b] is read.  out_stride should
 * be at least ttsamd_resample_out_len(handle, wave_stride): outputs past out_stride are dropped.
 * route: 0 automatic, 1 the general kernel (VALU; every handle), 2 the MFMA kernel (v_mfma_f32_16x16x4_f32, exact fp32; a block owns
 * 64 frames of one row and up to 256 phases).  Route 2 is eligible when n >= 16 and the block's LDS fits 160 KB: the skewed input strip,
 * (63 o + J') (1 + pad / o) floats with J' = J rounded up to 16 and pad = (4 - o mod 8) mod 8, plus two tap tiles of 16 x (32 NTW + 16 ..
 * 79) floats, NTW = ceil(n / (32 ceil(n / 256))); otherwise TTSAMD_EINVAL with a message.  Route 0 takes the MFMA kernel when it is
 * eligible and the launch has at least 48 of its blocks, else the general kernel (profiles/r12/NOTES.md). */
int32_t ttsamd_resample_forward(void* handle, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, float* out,
                                int64_t out_stride, int64_t* nout, int32_t route, void* stream);

/* librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length) per row, specified by its arithmetic: T = 1 + L / hop frames,
 * centred with zero padding of frame_length / 2 per side; ms_t = mean of the squares of frame t (fp32); r2_t = max(ms_t, 1e-10); frame t
 * is non-silent iff r2_t > 10^(-top_db / 10) max_t r2_t; with the first and last non-silent frames a, z: bounds[b] = (a hop,
 * min(L, (z + 1) hop)), (0, 0) when there is none.  peak [B] (may be NULL) = max |x| over the row, from the same pass.  gain > 0: the
 * bounds are those of the row scaled to that peak (ms_t (gain / peak)^2 in place of ms_t: what ttsamd_trim_apply writes; the scale only
 * moves the 1e-10 floor), gain = 0: of the row as given.  Limits: frame_length <= 8192, 1 <= hop_length <= frame_length.
 * workspace: ttsamd_trim_workspace_bytes(batch, wave_stride, hop_length) bytes (256-byte aligned; -1 for arguments the call refuses). */
int64_t ttsamd_trim_workspace_bytes(int32_t batch, int64_t wave_stride, int32_t hop_length);
int32_t ttsamd_trim_bounds(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, float top_db,
                           int32_t frame_length, int32_t hop_length, float gain, int64_t* bounds, float* peak, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* out[b][i] = fl32(fl32(wave[b][start + i] / peak[b]) * gain) for i < end - start (division first, then the multiplication, each rounded
 * to fp32 as numpy's float32 `x / m * gain`), zero from there to out_stride; peak NULL or peak[b] == 0: the row is copied unscaled.
 * lens_out int64 [B] (may be NULL) = min(end - start + tail, out_stride): `tail` zeros are counted into the length. */
int32_t ttsamd_trim_apply(const float* wave, int64_t wave_stride, const int64_t* bounds, const float* peak, float gain, int64_t tail,
                          int32_t batch, float* out, int64_t out_stride, int64_t* lens_out, void* stream);
/* The reference's remove_silence + mel_log[:, keep] / pitch[:, keep] per row: mel [B][C][t_max], lens int64 [B], extra [B][C2][t_max]
 * (may be NULL, then extra_out too).  e_t = the mean of frame t over the C channels (fp32, summed in channel order); keep_t = e_t > thresh;
 * every frame behind the last kept one is kept as well; with no frame above the threshold frames 1 .. T - 1 are kept and frame 0 is not
 * (the reference's loop, reproduced).  mel_out / extra_out (other buffers than the inputs): the kept columns in order, bit for bit, zero
 * from the new length to t_max; lens_out int64 [B] = the new lengths. */
int32_t ttsamd_frames_compact(const float* mel, const float* extra, const int64_t* lens, int32_t batch, int32_t n_channels,
                              int32_t n_extra, int32_t t_max, float thresh, float* mel_out, float* extra_out, int64_t* lens_out,
                              void* stream);

/* ---- Paragraph join (csrc/join.hip): the rows of a ragged batch of waves become ONE row -- each cut to its speech bounds, faded at
 * both edges, followed by an exact pause or overlap-added onto the next row -- before anything leaves the device.
 * All pointers are DEVICE pointers: wave fp32 [batch][wave_stride]; nsamples int64 [batch]; bounds int64 [batch][2] (what
 * ttsamd_trim_bounds writes) or NULL = whole rows; gap int64 [batch]: samples of silence behind row b (the last entry: the trailing
 * silence), negative = that many samples of overlap with the next row asked for (a gap above 2^40 is taken as 2^40); fade fp32
 * [n_fade]: a rising table, n_fade = 0 (fade may be NULL): no fades.  keep: samples kept outside the bounds on each side; lead: zeros in
 * front of the first row.  Specified by its arithmetic, matched bit for bit:
 *   1. source range: n_b = clamp(nsamples[b], 0, wave_stride); (s, e) = bounds[b] clamped to 0 <= s <= e <= n_b, (0, n_b) without
 *      bounds; if e > s: s = max(0, s - keep), e = min(n_b, e + keep); m_b = e - s.  A row with m_b = 0 gives no samples; its gap counts.
 *   2. effective gap: g_b = gap[b] where that is >= 0, else g_b = -min(-gap[b], n_fade, m_b / 2, m_{b+1} / 2) (integer halves); a
 *      negative gap of the last row is 0.  The halves leave at most two rows over any output sample.
 *   3. positions: p_0 = lead, p_{b+1} = p_b + m_b + g_b; total = p_{B-1} + m_{B-1} + g_{B-1}.
 *   4. fades: y_b[i] = fl32(fl32(x_b[i] fin(i)) fout(m_b - 1 - i)), x_b[i] = wave[b][s + i], fin(i) = fout(i) = fade[i] for i < n_fade,
 *      else 1; both act on rows shorter than 2 n_fade, and the first row fades in and the last fades out like every other.
 *   5. out[j] = y_b[j - p_b] of the one row with p_b <= j < p_b + m_b, fl32 of the sum of the two where two rows cover j (a two-term fp32
 *      sum does not depend on the order), 0 where none does; everything from `total` to out_stride is written as zero; samples at or
 *      past out_stride are dropped, and `total` and `segs` are reported unclamped so that the caller can tell (the resampler's convention).
 * out fp32 [out_stride]; segs int64 [batch][4] = (p_b, p_b + m_b, s, e): where row b lies in `out` and which of its samples went there;
 * total int64 [1].  Two launches whatever the batch (one block scans the rows; one gather over the output: plain dword loads, 16-byte
 * stores where out + j is aligned), no atomics, no host read-back; every source sample is read once and every output sample written
 * once; two runs give the same bits.
 * TTSAMD_EINVAL (nothing launched): batch outside 1 .. 4096, n_fade outside 0 .. 4096, a NULL wave / nsamples / gap / out / segs / total,
 * a NULL fade with n_fade > 0, a negative stride, keep or lead (or one of 2^40 and more). */
int32_t ttsamd_wave_join(const float* wave, int64_t wave_stride, const int64_t* nsamples, const int64_t* bounds, const int64_t* gap,
                         int32_t batch, const float* fade, int32_t n_fade, int64_t keep, int64_t lead, float* out, int64_t out_stride,
                         int64_t* segs, int64_t* total, void* stream);

/* ---- Token and word spans (csrc/timing.hip): per-token repeat counts -> where every token and every group of tokens (a word) lies in
 * the audio that is delivered.  A new symbol only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.
 * All pointers are DEVICE pointers: reps int64 [batch][reps_stride] (FastPitch's reps, MAS durations as integers; reps_stride >=
 * max_tokens); n_tokens int64 [batch] or NULL = max_tokens in every row, clamped to [0, max_tokens]; groups int32 [batch][max_groups][2]:
 * half-open token ranges (t0, t1), or NULL = no groups; n_groups int32 [batch] or NULL = max_groups in every row, clamped to
 * [0, max_groups]; hop: samples per repeat; map int64 [batch][5] = (lo, hi, off, num, den) per row, or NULL = (0, INT64_MAX, 0, 1, 1).
 * Specified by its arithmetic, in exact int64, matched bit for bit (n = the row's token count):
 *   1. c[0] = 0, c[i + 1] = c[i] + max(reps[i], 0) for i < n.
 *   2. m(p) = off + ceil((min(max(p hop, lo), hi) - lo) num / den): the position p hop of the row's own audio, cut to the part [lo, hi]
 *      that is kept, counted at num / den of the rate and moved to off.  The ceiling is the first delivered sample at or after the
 *      instant, the rule of the stream's chunk borders.  (p hop saturates at INT64_MAX; the result is exact where it fits int64.)
 *   3. tok[i] = (m(c[i]), m(c[i + 1])) for i < n, (m(c[n]), m(c[n])) for n <= i < max_tokens.
 *   4. grp[g] = (m(c[t0']), m(c[t1'])), t0' = clamp(t0, 0, n), t1' = max(clamp(t1, 0, n), t0') for g < n_groups[b]: an empty range is an
 *      empty span at its place; (m(c[n]), m(c[n])) for n_groups[b] <= g < max_groups.
 *   5. a row whose map has num or den outside [1, 2^20] or hi < lo gets -1 in all of its tok and grp entries; the other rows do not
 *      depend on it, and nothing faults.
 * tok int64 [batch][max_tokens][2]; grp int64 [batch][max_groups][2] (with groups, else NULL), both 16-byte aligned.  One launch, one
 * block per row (a wave64 shuffle scan per 64 tokens, carries through LDS and a register; c stays in LDS for the group pass), plain
 * vector stores, no atomics, no host read-back; two runs give the same bits.
 * TTSAMD_EINVAL (nothing launched, nothing written): batch < 1, max_tokens outside 1 .. 8192, reps_stride < max_tokens, max_groups < 0,
 * hop < 1 (or 2^31 and more), a NULL reps / tok, groups without grp or grp without groups, a tok / grp that is not 16-byte aligned. */
#define TTSAMD_SPANS_MAX_TOKENS 8192
int32_t ttsamd_token_spans(const int64_t* reps, int64_t reps_stride, const int64_t* n_tokens, int32_t batch, int32_t max_tokens,
                           const int32_t* groups, const int32_t* n_groups, int32_t max_groups, int64_t hop, const int64_t* map,
                           int64_t* tok, int64_t* grp, void* stream);

/* ---- Tacotron2MS.infer: replaces models/tacotron2/tacotron2_ms.py:279-332 (encoder, speaker
 *      concat, autoregressive _Decoder.infer, postnet).  Weight names are the keys of
 *      Tacotron2MS.state_dict() (embedding.weight, speaker_embedding.weight, encoder.*, decoder.*,
 *      postnet.*); BatchNorm layers are folded on the host (eval mode). --------------------------- */
int32_t ttsamd_tacotron2_create(const ttsamd_tensor* weights, int32_t n_weights,
                                const ttsamd_tacotron2_cfg* cfg, void** handle);
int32_t ttsamd_tacotron2_destroy(void* handle);
int64_t ttsamd_tacotron2_workspace_bytes(void* handle, int32_t batch, int32_t n_tokens, int32_t max_step);
/* tokens int64 [B][n_tokens] (zero-padded), lengths int64 [B] sorted descending or not (packed-sequence
 * semantics per utterance), speaker_ids int64 [B] or NULL (num_speakers == 1); all DEVICE pointers.
 * Outputs (device): mel_post / mel_raw [B][n_mels][max_step] (row stride max_step; frames >= *n_steps
 * are untouched), mel_lens int32 [B], alignments [B][max_step][n_tokens].  *n_steps (HOST) = number of
 * decoder steps the reference loop would have run (it stops once every utterance's gate fired, or at
 * max_step).  dropout_seed < 0 disables the prenet dropout; >= 0 applies the always-on p=0.5 dropout of
 * torchaudio's _Prenet with a counter-based hash (seed, layer, step, b, j) instead of torch's RNG. */
int32_t ttsamd_tacotron2_infer(void* handle, const int64_t* tokens, const int64_t* lengths,
                               const int64_t* speaker_ids, int32_t batch, int32_t n_tokens, int32_t max_step,
                               int64_t dropout_seed, float* mel_post, int32_t* mel_lens, float* alignments,
                               float* mel_raw, int32_t* n_steps, void* workspace, int64_t workspace_bytes,
                               void* stream);

/* ---- Tacotron2 as a stream: the same decode in advances of a few steps, so that audio can leave while the decoder is still running
 *      (no reference counterpart; ttsamd/engine.py Tacotron2Engine.stream, models/tacotron2/networks.py Tacotron2Wave.tts_stream).
 *      New entries at ABI revision 8; the handle is not changed by a session.  Device state lives in the caller's `workspace`
 *      (ttsamd_tacotron2_stream_bytes: the exchange arena is sized by max_chunk_steps, not by max_step, and there are no postnet
 *      buffers in it) and in the caller's output buffers, all of which must stay alive and untouched until ttsamd_tacotron2_stream_end;
 *      the small host side (the decoder path, the step position, the captured step graph of the graph path) is *session. ----------- */
int64_t ttsamd_tacotron2_stream_bytes(void* handle, int32_t batch, int32_t n_tokens, int32_t max_step, int32_t max_chunk_steps);
/* The head of ttsamd_tacotron2_infer (encoder, speaker concat, processed memory, the zero decoder state) and the choice of the decoder
 * path, made once by infer's own rule (persistent where it fits, TTSAMD_TACO_PERSISTENT as there).  tokens / lengths / speaker_ids /
 * mel_raw / mel_lens / alignments: as ttsamd_tacotron2_infer (device; row strides max_step).  max_chunk_steps: the longest advance, a
 * positive multiple of 8.  cut_columns int32 [B] (device, copied; may be NULL = no row has one): per row the token column whose
 * attention weights define the wrapper's end-of-utterance cut (truncate_mel), < 0 = none.  rows_to_batch_end != 0: a row ends with the
 * batch and is as long as the batch (Tacotron2.ttmel_single's rule); 0: a row ends at its own mel_lens (ttmel_batch's). */
int32_t ttsamd_tacotron2_stream_begin(void* handle, const int64_t* tokens, const int64_t* lengths, const int64_t* speaker_ids, int32_t batch,
                                      int32_t n_tokens, int32_t max_step, int32_t max_chunk_steps, int64_t dropout_seed,
                                      const int32_t* cut_columns, int32_t rows_to_batch_end, float* mel_raw, int32_t* mel_lens,
                                      float* alignments, void* workspace, int64_t workspace_bytes, void** session, void* stream);
/* Steps [s, s + n_steps) of the same loop, clipped to max_step: one cooperative launch on the persistent path, n_steps / 8 replays of a
 * graph captured once per session on the graph path; the frames and alignments written are ttsamd_tacotron2_infer's bit for bit.
 * n_steps: a positive multiple of 8, at most max_chunk_steps.  HOST outputs (the call waits for the steps): *ended = every row's gate has
 * fired (with decoder_early_stopping) or max_step is reached; *steps_done = the steps ttsamd_tacotron2_infer would report so far;
 * rows int32 [B][4] (may be NULL) = per row { final_frames, row_ended, n_end, row_length }:
 *   n_end        the cut bound c_s = the first t < s with ps[t] >= 0.8f * max(ps[:s]) over the row's cut column (never decreases, never
 *                exceeds truncate_mel's cut, and is that cut once row_ended); the row length for a row without a column
 *   final_frames min(n_end, frames whose postnet output is settled: t + halo < steps computed, or all of them once ended)
 *   row_ended    the row's length is known (a gate that fires on the very last step of an advance shows one advance later, or with *ended)
 * A hand-off time-out of a persistent segment (as in ttsamd_tacotron2_infer) replays steps [0, s + n_steps) on the graph path and the
 * session stays there; under an explicit TTSAMD_TACO_PERSISTENT=1 / 2 it is an error.  After *ended a further call is TTSAMD_EINVAL. */
int32_t ttsamd_tacotron2_stream_advance(void* session, int32_t n_steps, int32_t* steps_done, int32_t* ended, int32_t* rows, void* stream);
int32_t ttsamd_tacotron2_stream_end(void* session);
/* The postnet over windows.  *halo = postnet_n_convolution * (postnet_kernel_size - 1) / 2 frames (10): what an output frame reads on
 * each side.  ttsamd_tacotron2_postnet_window writes mel_post[:, :, t0:t1) from the raw frames [t0 - halo, t1 + halo) clipped to
 * [0, t_known): zero padding falls where the one-shot postnet has it -- at frame 0, and at t_known when `ended` is set (t_known is then the
 * step count of the decode) -- and nowhere else: t1 + halo > t_known with ended == 0 is TTSAMD_EINVAL.  A row that finished early reads
 * the frames decoded after its gate fired, as the one-shot postnet on the padded batch does.  mel_raw / mel_post [B][n_mels][t_cap];
 * workspace: ttsamd_tacotron2_postnet_window_bytes(handle, batch, t1 - t0). */
int32_t ttsamd_tacotron2_postnet_halo_frames(void* handle, int32_t* halo);
int64_t ttsamd_tacotron2_postnet_window_bytes(void* handle, int32_t batch, int32_t n_frames);
int32_t ttsamd_tacotron2_postnet_window(void* handle, const float* mel_raw, float* mel_post, int32_t batch, int32_t t_cap, int32_t t_known,
                                        int32_t t0, int32_t t1, int32_t ended, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- diacritizer taggers: replaces Shakkelha.forward / Shakkala.forward
 *      (models/diacritizers/shakkelha/network.py:29-42, shakkala/network.py:31-43).  Weight names are
 *      canonical: emb.weight, lstm<i>.{weight,bias}_{ih,hh}_l0[_reverse], bn0.{weight,bias,running_mean,
 *      running_var}, dense<i>.{weight,bias} (the Python classes rename emb0 / emb_input). ------------------ */
int32_t ttsamd_tagger_create(const ttsamd_tensor* weights, int32_t n_weights, const ttsamd_tagger_cfg* cfg,
                             void** handle);
int32_t ttsamd_tagger_destroy(void* handle);
int64_t ttsamd_tagger_workspace_bytes(void* handle, int32_t batch, int32_t n_chars);
/* ids int64 [B][n_chars] (device) -> probs [B][n_chars][n_classes] (device), softmax over the classes.
 * Sequences run over the full n_chars in both directions (no packing), as the reference modules do. */
int32_t ttsamd_tagger_forward(void* handle, const int64_t* ids, int32_t batch, int32_t n_chars, float* probs,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* ---- kernel-level entry used by the parity tests and the roofline bench ------------- */

/* One Conv1d through the implicit-GEMM MFMA kernel: y = conv1d(lrelu_slope(x), w) + b.
 * x [B][Cin][Lin], w [Cout][Cin][K] (torch layout, DEVICE), y [B][Cout][Lin] ("same"
 * padding (K*dil-dil)/2), lens int64 [B] or NULL.  Allocates nothing; `packed` must hold
 * ttsamd_conv1d_packed_floats(Cout,Cin,K) floats of scratch for the re-laid-out weights. */
int64_t ttsamd_conv1d_packed_floats(int32_t cout, int32_t cin, int32_t k);
int32_t ttsamd_conv1d(const float* x, const float* w, const float* bias, const int64_t* lens,
                      int32_t batch, int32_t cin, int32_t cout, int32_t k, int32_t dilation,
                      int32_t lin, float in_slope, int32_t relu_out, float* y, float* packed,
                      void* stream);
/* the same with the rest of the conv engine's epilogue: y = act(conv + bias + res) | y + ... | (y + ...) / div  (mode 0 | 1 | 2); res
 * [B][Cout][lin] or NULL.  Drives the residual-preload epilogues of the direct and the Winograd F(2,3) kernel (csrc/conv_wino.hip:
 * k = 3, dilation 1 launches of at least one 128 x 128 tile per CU; TTSAMD_WINO=0 keeps the direct kernel) in the parity tests. */
/* (relu_out != 0 is defined for mode 0 only: with an accumulate mode the call returns TTSAMD_EINVAL) */
int32_t ttsamd_conv1d_ex(const float* x, const float* w, const float* bias, const float* res, const int64_t* lens, int32_t batch,
                         int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope,
                         int32_t relu_out, int32_t mode, float div, float* y, float* packed, void* stream);
/* ---- the launches a model forward takes at batch 1, for the parity tests.  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION
 *      stays 8; ttsamd_conv1d_ex is ttsamd_conv1d_splitk(..., NULL, 0, ...), bit for bit what it was.
 * ttsamd_conv1d_splitk: ttsamd_conv1d_ex with the split-K workspace the models hand their convs (ConvParams::splitk_ws): `splitk_ws` =
 * `splitk_floats` floats of device scratch, or NULL / 0.  With it a launch of few blocks cuts its input channels into slices (direct
 * kernel: under 320 blocks and from 8 chunks; F(4,3) kernel: under 192 blocks), each slice writes raw partial sums
 * [slice][B][Cout][lin] into the workspace and a second launch sums them in slice order and applies the epilogue.  No more slices than
 * the workspace holds: under 2 * B * Cout * lin floats nothing is split.  The models pass 4 << 20 floats (FastPitch: 8 << 20). */
int32_t ttsamd_conv1d_splitk(const float* x, const float* w, const float* bias, const float* res, const int64_t* lens, int32_t batch,
                             int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope,
                             int32_t relu_out, int32_t mode, float div, float* y, float* packed, float* splitk_ws, int64_t splitk_floats,
                             void* stream);
/* What the calling thread's last fp32 conv launch decided (ttsamd_conv1d*, ttsamd_conv_transpose1d, or the last conv of a model forward
 * on this thread): *route = 0 direct kernel, 1 / 2 the two Winograd F(2,3) kernels, 3 / 4 Winograd F(4,3) on six- / seven-point groups,
 * 5 the all-phase transposed conv, 6 the transposed conv as a two-tap conv on Winograd F(4,2), 7 / 8 Winograd F(4,3) on six- / seven-point
 * groups in the packed strip form (dilation 3 / 5, one C-in slice, no residual, mode 0; TTSAMD_WINO4 bit 7); *ksplit = its input-channel slices (1 = not split).  -1 / 0 before the first launch.  Host state of
 * the thread only: nothing is read from the device.  The bf16 engines and the fused ResBlock launches do not record. */
int32_t ttsamd_conv_last_launch(int32_t* route, int32_t* ksplit);
/* Asks without launching (new symbol, added WITHOUT a bump; host only, needs no GPU): the (*route, *ksplit) that ttsamd_conv_last_launch
 * would report after ttsamd_conv1d_splitk with these arguments under the current options, for 16-byte aligned x / y / res (has_res != 0:
 * a residual is passed) and a workspace of splitk_floats floats (0: none).  TTSAMD_EINVAL where that call would be rejected, and under the
 * bf16 precisions, whose launchers keep their own choices. */
int32_t ttsamd_conv1d_route(int32_t batch, int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope,
                            int32_t relu_out, int32_t has_res, int32_t mode, int64_t splitk_floats, int32_t* route, int32_t* ksplit);
/* One HiFi-GAN upsampler (vocoder/hifigan/models.py:96-99, 114-115) as the generator runs it: y = conv_transpose1d(lrelu_slope(x), w,
 * stride u, padding u / 2) + b with the kernel size 2 u (u even), the only form the engine packs.  x [B][Cin][lin] (Cin a multiple of
 * 8), w [Cin][Cout][2u] (torch layout, DEVICE), y [B][Cout][lin * u], bias [Cout] or NULL, lens int64 [B] or NULL: row b reads lens[b]
 * inputs and writes lens[b] * u outputs; y past them is left untouched (both kernels, as for ttsamd_conv1d; the generator's next layers
 * never read there).  The all-phase kernel (csrc/convt_mfma.hip; route 5) takes u = 2 / 8 with 16-byte aligned rows of y and, at u = 8,
 * at least 100 blocks; everything else, and everything under TTSAMD_CONVT=0, is the direct kernel's polyphase launch (route 0).
 * In fp32, u = 2 / 8 with Cin a multiple of 16, u Cout a multiple of 64 and 16-byte aligned rows of x and y can also run as a two-tap
 * conv with u Cout rows on Winograd F(4,2) (csrc/conv_wino4.hip; route 6): TTSAMD_CONVT_WINO=2 wherever that holds, =1 / unset only
 * the (Cin, u) classes and sizes the generator routes there by default (batch x lin >= 8192), =0 never.
 * `packed`: ttsamd_convt_packed_floats(Cin, Cout, u) floats of scratch for the re-laid-out weights. */
int64_t ttsamd_convt_packed_floats(int32_t cin, int32_t cout, int32_t u);
/* HOST: the weights of that F(4,2) launch as the generator keeps them -- w [Cin][Cout][2u] (torch layout, host), bias [Cout] or NULL ->
 * out[0 .. 6 Cin u Cout): the group filters U0..U4 and a zero group of the taps (w[..][j + u], w[..][j], 0), row = co u + j, as
 * [Cin/8][6][2][u Cout][4]; behind them u Cout floats: the bias per row.  ttsamd_convt_wino_packed_floats = (6 Cin + 1) u Cout, 0 for a
 * shape the launch does not take (then ttsamd_convt_wino_pack_weight is TTSAMD_EINVAL).  No GPU needed. */
int64_t ttsamd_convt_wino_packed_floats(int32_t cin, int32_t cout, int32_t u);
int32_t ttsamd_convt_wino_pack_weight(const float* w, const float* bias, int32_t cin, int32_t cout, int32_t u, float* out);
int32_t ttsamd_conv_transpose1d(const float* x, const float* w, const float* bias, const int64_t* lens, int32_t batch, int32_t cin,
                                int32_t cout, int32_t u, int32_t lin, float in_slope, float* y, float* packed, void* stream);

/* One c1 -> c2 pair of a ResBlock1 (vocoder/hifigan/models.py:46-53) in exact fp32, intermediate in LDS:
 *   v = x + conv1d(lrelu(conv1d(lrelu(x, slope), w1, dilation dil) + b1, slope), w2) + b2;  y = v | y + v | (y + v) / div  (mode 0 | 1 | 2)
 * x, y [B][C][L] (y != x), w1 / w2 [C][C][K] (torch layout, DEVICE), lens int64 [B] or NULL (valid length lens[b] * len_mul:
 * every conv pads at the true edge).  variant 1: first-generation kernel (weights through an LDS ring; C = 32, or C = 64 with
 * k = 3), 2 / 3: second generation (weights from L2 into a register queue, raw window; 256- / 128-column blocks; C = 32 / 64 /
 * 128, k = 3 / 7 / 11), 4 / 5: 256-column blocks with conv 2 (4) or both convs (5) on Winograd F(2,3) (C = 32 / 64, k = 3 / 7 / 11;
 * 5 also C = 128), 6: C = 32 with both convs on Winograd F(4,3) (512-column blocks, k = 3 / 7 / 11, dilation 1 / 3 / 5; L a multiple
 * of 4), 7: the same launch with both convs on its seven-point groups (13 / 20 products per output quad; C = 32, k = 7 / 11 only).
 * `packed` is scratch for the re-laid-out weights: ttsamd_resblock_pair_packed_floats(C, K, variant) floats (the two
 * direct packings, + the Winograd group filters of variants 4 / 5 / 6 / 7); `packed_floats` = what the caller allocated, a smaller buffer is
 * TTSAMD_EINVAL (nothing is written). */
int64_t ttsamd_resblock_pair_packed_floats(int32_t channels, int32_t k, int32_t variant);
int32_t ttsamd_resblock_pair(const float* x, float* y, const float* w1, const float* b1, const float* w2, const float* b2,
                             int32_t channels, int32_t k, int32_t dil, const int64_t* lens, int32_t len_mul, int32_t L,
                             int32_t batch, int32_t mode, float div, float slope, int32_t variant, float* packed, int64_t packed_floats,
                             void* stream);
/* Asks without launching (new symbol, added WITHOUT a bump; host only, needs no GPU): what ttsamd_hifigan_forward launches under the
 * current options and precision for the c1 -> c2 pair of a ResBlock1 with C channels, kernel size k and this dilation at a stage of L
 * positions per row and `batch` rows, packed as ttsamd_hifigan_create packs it, on 16-byte aligned, distinct buffers.  *kernel: 0 two
 * conv launches (ttsamd_conv1d_route says which), 1 first-generation fused pair, 2 second generation (*ntw = 2 / 1: 256- / 128-column
 * blocks; *wino_phases = 0 / 1 / 2: none, conv 2, both convs on Winograd F(2,3)), 3 both convs on Winograd F(4,3) (*points = 6 / 7:
 * six- / seven-point groups).  *name: the kind TTSAMD_CONV_LOG records for the launch ("" for kernel 0; a static string). */
int32_t ttsamd_resblock_pair_route(int32_t batch, int32_t channels, int32_t k, int32_t dilation, int32_t L, int32_t* kernel, int32_t* ntw,
                                   int32_t* wino_phases, int32_t* points, const char** name);

/* One ResBlock2 (vocoder/hifigan/models.py:62-83) in exact fp32:
 *   x1 = x + conv1d(lrelu(x, slope), w1, dilation dil1) + b1;  v = x1 + conv1d(lrelu(x1, slope), w2, dilation dil2) + b2;
 *   y = v | y + v | (y + v) / div  (mode 0 | 1 | 2)
 * x, y [B][C][L] (y != x), w1 / w2 [C][C][K] (torch layout, DEVICE), lens int64 [B] or NULL: every conv zero-pads at the true edge
 * lens[b] * len_mul and nothing past it is written.  variant 1: two single-conv launches (C = 32 / 64 / 128, k = 3 / 5 / 7 / 11,
 * dilation 1..16; x1 goes through a stream-ordered temporary of B * C * L floats), 2: both convs in one launch with x1 in LDS (C = 32 /
 * 64, k = 3 / 5 / 7 / 11, dilation 1..16, (k - 1) * dil2 <= 256).  A geometry the variant does not cover is TTSAMD_EINVAL.  `packed` is
 * scratch for the re-laid-out weights: ttsamd_resblock2_packed_floats(C, K, variant) floats; a smaller `packed_floats` is TTSAMD_EINVAL. */
int64_t ttsamd_resblock2_packed_floats(int32_t channels, int32_t k, int32_t variant);
int32_t ttsamd_resblock2(const float* x, float* y, const float* w1, const float* b1, const float* w2, const float* b2, int32_t channels,
                         int32_t k, int32_t dil1, int32_t dil2, const int64_t* lens, int32_t len_mul, int32_t L, int32_t batch, int32_t mode,
                         float div, float slope, int32_t variant, float* packed, int64_t packed_floats, void* stream);

/* ---- bf16 octet engine (BASELINE config 3), kernel-level entries used by the parity tests and the roofline bench.
 *      Activations are [B][C/8][L][8] bf16 ("octet" layout: one 16-byte entry = 8 channels of one position = one lane's B
 *      operand of v_mfma_f32_32x32x16_bf16), stored PRE-ACTIVATED: a = leaky_relu(x, slope of the consumer).  Replaces
 *      ResBlock1.forward / Generator.forward's convs (vocoder/hifigan/models.py:46-53, 111-127) when
 *      ttsamd_set_precision(1) is in force; ttsamd_hifigan_forward routes through it by itself. ------------------------- */
/* fp32 channel-first [B][C][len] -> octet bf16 with leaky_relu(slope) applied (slope 1 = raw); and back (inverse applied) */
int32_t ttsamd_bfo_pack(const float* x, int32_t batch, int32_t channels, int32_t len, float slope, void* out, void* stream);
int32_t ttsamd_bfo_unpack(const void* in, int32_t batch, int32_t channels, int32_t len, float slope, float* out, void* stream);
/* HOST: torch Conv1d weight [Cout][Cin][K] (up = 1) or ConvTranspose1d weight [Cin][Cout][2*up] (stride up, padding up/2)
 * -> bf16 [phases][Cin/16][K][2][CoutP][8]; `out` holds ttsamd_bfo_weight_elems(...) uint16 */
int64_t ttsamd_bfo_weight_elems(int32_t cout, int32_t cin, int32_t k, int32_t up);
int32_t ttsamd_bfo_pack_weight(const float* w, int32_t cout, int32_t cin, int32_t k, int32_t up, uint16_t* out);
/* y = act_out(([sum_in +] conv(x) + bias [+ raw(res)]) [/ div]): x, res activated tensors, sum_in raw; mode as below;
 * out_slope 0 = ReLU.  up > 1: ConvTranspose1d(stride up), y has len_in * up positions (no res / sum).
 * y_f32 != NULL: the result leaves as fp32 channel-first [B][Cout][len] instead of y, res_f32 (NULL = none) is an fp32
 * channel-first residual: FastPitch's Conv1d + ReLU -> Conv1d + residual block (models/fastpitch/fastpitch/transformer.py:72-90)
 * keeps its residual stream in fp32 and only the 1536-channel intermediate in bf16. */
int32_t ttsamd_bfo_conv1d(const void* x, const void* w_packed, const float* bias, const void* res, const void* sum_in,
                          const int64_t* lens, int32_t len_mul, int32_t batch, int32_t cin, int32_t cout, int32_t k,
                          int32_t dilation, int32_t up, int32_t len_in, int32_t mode, float div, float res_slope,
                          float out_slope, void* y, float* y_f32, const float* res_f32, void* stream);
/* one c1 -> c2 pair of ResBlock1 (models.py:46-53) in one launch, C in {32, 64, 128}, k in {3, 7, 11}:
 *   v = raw(x) + conv(lrelu(conv(x, w1, dilation) + b1, mid_slope), w2) + b2
 *   mode 0: y = act(v)   1: y = act(sum_in + v)   2: y = act((sum_in + v) / div);   act = leaky_relu(out_slope), 1 = raw.
 * x is stored activated with in_slope; y must not alias x. */
int32_t ttsamd_bfo_resblock_pair(const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                                 const void* sum_in, const int64_t* lens, int32_t len_mul, int32_t batch, int32_t channels,
                                 int32_t k, int32_t dilation, int32_t len, int32_t mode, float div, float in_slope,
                                 float mid_slope, float out_slope, void* y, void* stream);
/* a whole k = 3 ResBlock1 (the three pairs of models.py:46-53 with dilations[0..2], C in {32, 64, 128}) in one launch; w1 / b1 / w2 /
 * b2 are arrays of three device pointers.  Equals three ttsamd_bfo_resblock_pair calls (out_slope = in_slope between them, mode /
 * sum_in / out_slope on the last) bit for bit. */
int32_t ttsamd_bfo_resblock_chain(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                                  const float* const* b2, const int32_t* dilations, const void* sum_in, const int64_t* lens,
                                  int32_t len_mul, int32_t batch, int32_t channels, int32_t len, int32_t mode, float div,
                                  float in_slope, float mid_slope, float out_slope, void* y, void* stream, int32_t k);
/* wave[b][t] = tanh(bias + conv7(x)); x = 32-channel octet tensor already activated with slope 0.01 (models.py:123-125) */
int32_t ttsamd_bfo_conv_post(const void* x, const float* w, const float* bias, const int64_t* lens, int32_t len_mul,
                             int32_t batch, int32_t channels, int32_t len, float* wave, int64_t wave_stride, void* stream);

/* ---- split-bf16 ("x3") mode of the octet engine: the same layers with fp32-class results (north_star's 1e-3 / 1e-4), every
 *      value = hi + lo (two bf16), three v_mfma_f32_32x32x16_bf16 per product (Wh xh + Wh xl + Wl xh, fp32 accumulate).
 *      Activations ("x3 tensor"): [B][C/8][L][2][hi 4 bf16 | lo 4 bf16] = 32 bytes per (octet, position) -- the 16-byte half kk
 *      holds channels 8o + 4kk + {0..3}, one lane's slice of the MFMA C layout -- stored PRE-ACTIVATED like the bf16 tensors.
 *      Weights: [phases][Cin/16][K][2][CoutP][hi 8 | lo 8] bf16.  Same argument meanings as the ttsamd_bfo_* twins above;
 *      ttsamd_hifigan_forward / ttsamd_fastpitch_* route through these kernels under ttsamd_set_precision(2).
 *      Ops: vocoder/hifigan/models.py:46-53, 96-99, 111-127. ------------------------------------------------------------------- */
int32_t ttsamd_bfo3_pack(const float* x, int32_t batch, int32_t channels, int32_t len, float slope, void* out, void* stream);
int32_t ttsamd_bfo3_unpack(const void* in, int32_t batch, int32_t channels, int32_t len, float slope, float* out, void* stream);
int64_t ttsamd_bfo3_weight_elems(int32_t cout, int32_t cin, int32_t k, int32_t up);
int32_t ttsamd_bfo3_pack_weight(const float* w, int32_t cout, int32_t cin, int32_t k, int32_t up, uint16_t* out);
int32_t ttsamd_bfo3_conv1d(const void* x, const void* w_packed, const float* bias, const void* res, const void* sum_in,
                           const int64_t* lens, int32_t len_mul, int32_t batch, int32_t cin, int32_t cout, int32_t k,
                           int32_t dilation, int32_t up, int32_t len_in, int32_t mode, float div, float res_slope,
                           float out_slope, void* y, float* y_f32, const float* res_f32, void* stream);
int32_t ttsamd_bfo3_resblock_pair(const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                                  const void* sum_in, const int64_t* lens, int32_t len_mul, int32_t batch, int32_t channels,
                                  int32_t k, int32_t dilation, int32_t len, int32_t mode, float div, float in_slope,
                                  float mid_slope, float out_slope, void* y, void* stream);
/* a whole k = 3 ResBlock1 (three pairs, dilations[0..2]) in one launch; equals three ttsamd_bfo3_resblock_pair calls bit for bit */
int32_t ttsamd_bfo3_resblock_chain(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                                   const float* const* b2, const int32_t* dilations, const void* sum_in, const int64_t* lens,
                                   int32_t len_mul, int32_t batch, int32_t channels, int32_t len, int32_t mode, float div,
                                   float in_slope, float mid_slope, float out_slope, void* y, void* stream);
int32_t ttsamd_bfo3_conv_post(const void* x, const float* w, const float* bias, const int64_t* lens, int32_t len_mul,
                              int32_t batch, int32_t channels, int32_t len, float* wave, int64_t wave_stride, void* stream);

/* MFMA operand precision of every conv/linear GEMM launched by the model forwards (process-wide):
 *   0 (default) exact fp32 (v_mfma_f32_32x32x2_f32) — BASELINE config 2;
 *   1 bf16 operands, fp32 accumulate — config 3: HiFi-GAN on the octet engine above (v_mfma_f32_32x32x16_bf16, bf16
 *     activations in HBM), the other models on v_mfma_f32_32x32x8_bf16_1k with fp32 activations;
 *   2 split bf16 (x = hi + lo, 3 MFMAs per product): fp32-class accuracy at bf16 MFMA rate.
 * A ResBlock2 (V3) HiFi-GAN generator is built for fp32 only: ttsamd_hifigan_forward refuses it under 1 / 2 (TTSAMD_EINVAL).
 * Activations, LayerNorm, softmax, tanh, the FFTs and all integer work stay fp32/int64. */
int32_t ttsamd_set_precision(int32_t precision);
int32_t ttsamd_get_precision(void);

/* ---- data-parallel sharding over the GPUs of one node: RCCL over xGMI.
 *      No reference counterpart: the reference is single-device (inference.py:23-24); utterances are
 *      independent, so the only exchanges are C1 (weights, once) and C2 (lengths + audio fan-in per call).
 *      One communicator per process (= per GPU); librccl.so.1 is bound at run time by the first call.
 *      Host binding (ctypes / cgo / JNI alike): rank 0 calls ttsamd_dp_unique_id and ships the 128 bytes
 *      to the other ranks out of band (env, file, torch.distributed store); every rank then calls
 *      ttsamd_dp_init after hipSetDevice(local_rank). ------------------------------------------------- */
#define TTSAMD_DP_ID_BYTES 128
#define TTSAMD_DP_HIFIGAN 0
#define TTSAMD_DP_FASTPITCH 1
int32_t ttsamd_dp_unique_id(void* id128 /* host, out */);
int32_t ttsamd_dp_init(int32_t rank, int32_t world, const void* id128 /* host */, void** comm);
int32_t ttsamd_dp_destroy(void* comm);
int32_t ttsamd_dp_rank(void* comm);
int32_t ttsamd_dp_world(void* comm);
/* C1, generic: in-place broadcast of a device buffer from `root`. */
int32_t ttsamd_dp_broadcast(void* comm, void* buf, int64_t nbytes, int32_t root, void* stream);
/* C1, handle form: overwrites this rank's packed weight blobs (fp32 + bf16 planes) of a
 * ttsamd_hifigan / ttsamd_fastpitch handle (kind = TTSAMD_DP_*) with the root's.  Non-root ranks create
 * their handle from tensors of the same names and shapes (any values): only rank 0 reads the checkpoint
 * (replaces one torch.load + remove_weight_norm per GPU; vocoder/__init__.py:15-18). */
int32_t ttsamd_dp_broadcast_weights(void* comm, int32_t kind, void* handle, int32_t root, void* stream);
/* C2a: recv[r*nbytes .. (r+1)*nbytes) = rank r's send[0 .. nbytes) on every rank (the lengths). */
int32_t ttsamd_dp_allgather(void* comm, const void* send, void* recv, int64_t nbytes_per_rank, void* stream);
/* C2b: packed[off(b) + t] = wave[b][t] for t < min(nsamples[b], n_max), off(b) = sum of the shorter-indexed
 * utterances' sample counts: the valid samples of a padded ragged batch back to back (no padding crosses
 * xGMI or PCIe).  wave [B][wave_stride], nsamples int64 [B] (device).  Needs no communicator. */
int32_t ttsamd_dp_pack_audio(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch,
                             int64_t n_max, float* packed, void* stream);
/* C2c: fan-in to `root`: rank r's packed[0 .. counts[r]) lands at recv[offsets[r] ..) on the root
 * (grouped ncclSend / ncclRecv: world-1 independent point-to-point transfers, one per xGMI link).
 * counts / offsets are HOST int64 [world] (floats), identical on every rank — the caller knows them from
 * the all-gathered lengths; recv / offsets are ignored on the other ranks. */
int32_t ttsamd_dp_gather_audio(void* comm, const float* packed, float* recv, const int64_t* counts,
                               const int64_t* offsets, int32_t root, void* stream);

/* ---- Streaming synthesis: chunked HiFi-GAN over windows of many open utterances (csrc/stream.hip; ttsamd/stream.py is the scheduler).
 *      No reference counterpart: the reference vocodes whole utterances.  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays
 *      8.  The generator is a stack of zero-padded convolutions, so a window of mel frames with `halo` extra frames per side (fewer
 *      where the utterance ends sooner: a window that touches an utterance edge starts or ends exactly there) gives on its core the
 *      samples of the whole-utterance call.  One step of the scheduler is gather -> forward of the HiFi-GAN handle -> denoise_rows of the
 *      denoiser (optional) -> emit, all on one stream, no host synchronisation.
 * The receptive field of the handle's generator in mel frames per side, from its own config: walking back from one frame of samples,
 * conv_post widens the sample interval by 3, every stage by its longest ResBlock branch (ResBlock1: the sum over m of (k - 1) / 2 *
 * (d_m + 1); ResBlock2: (k - 1) / 2 * (d_0 + d_1)), every transposed conv (kernel kt, stride u, padding p = (kt - u) / 2) maps
 * [lo, hi] to [ceil((lo + p - kt + 1) / u), floor((hi + p) / u)], conv_pre widens by 3.  13 / 13 for the V1 config. */
int32_t ttsamd_hifigan_halo_frames(void* handle, int32_t* left /* host, out */, int32_t* right /* host, out */);
/* ... and of the bias denoiser, in frames of 256 samples: a sample's STFT frames reach 512 samples to either side and their inverse
 * transforms another 512 back, so a sample depends on 768 to either side: 3 for the 1024 / 256 STFT, the only one the library builds. */
int32_t ttsamd_denoiser_halo_frames(void);
/* The most windows one gather / emit call takes (the descriptors travel as launch arguments: no staging copy, no synchronisation). */
#define TTSAMD_STREAM_MAX_WINDOWS 64
/* pool [n_slots][num_mels][t_cap] fp32 (one slot per open utterance) -> batch [n_windows][num_mels][w_max] fp32 and lens int64
 * [n_windows] (device; may be NULL), which is what the forward of the HiFi-GAN handle takes: window w holds frames [start[w], start[w] + len[w])
 * of slot slot[w]; columns past len[w] are written as zeros, lens[w] = len[w].  slot / start / len: HOST int32 [n_windows], read
 * during the call.  Required: 1 <= n_windows <= TTSAMD_STREAM_MAX_WINDOWS, 0 <= slot < n_slots, 0 <= start, 1 <= len <= w_max,
 * start + len <= t_cap; anything else is TTSAMD_EINVAL and nothing is launched.  The kernel reads nothing outside those windows. */
int32_t ttsamd_stream_gather(const float* pool, int32_t n_slots, int32_t num_mels, int32_t t_cap, const int32_t* slot /* host */,
                             const int32_t* start /* host */, const int32_t* len /* host */, int32_t n_windows, int32_t w_max,
                             float* batch, int64_t* lens, void* stream);
/* wave [n_windows][hop * w_max] fp32 (the window waves) -> out [n_windows][c_max]: row w = samples [core_off[w], core_off[w] +
 * core_len[w]) of wave row w, zeros behind them.  core_off / core_len: HOST int32 [n_windows] in SAMPLES, multiples of hop,
 * 0 <= core_off, 0 <= core_len <= c_max, core_off + core_len <= hop * w_max; hop and c_max multiples of 8, wave and out 16-byte
 * aligned (16-byte loads, packed stores); anything else is TTSAMD_EINVAL and nothing is launched.
 * format 0: out is fp32, a copy.  format 1: out is little-endian int16 PCM, clip(rint(x * 32767), -32768, 32767) with the product in
 * fp32 and the rounding to nearest even (numpy's np.round of the fp32 product), NaN -> 0. */
int32_t ttsamd_stream_emit(const float* wave, int32_t n_windows, int32_t w_max, int32_t hop, const int32_t* core_off /* host */,
                           const int32_t* core_len /* host */, int32_t c_max, int32_t format, void* out, void* stream);
/* Stream delivery formats: ttsamd_stream_emit with the polyphase resampler of ttsamd_resample_create and an encoder between the window
 * waves and the chunk rows.  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.
 * resample_handle: a handle of ttsamd_resample_create (o, n, width, J = 2 * width + o and its device table), or NULL for "rate
 * unchanged", which behaves as o = n = 1, width = 0 and one tap of 1.0.  wave [n_windows][hop * w_max] fp32 as for ttsamd_stream_emit.
 * Five HOST int32 arrays [n_windows], read during the call, all in SAMPLES OF THE UTTERANCE: win_start[w] = the utterance index of the
 * row's sample 0, win_len[w] = the valid samples of the row, utt_len[w] = L, core_start[w] = S0, core_end[w] = S1, with
 * 0 <= win_start <= S0 < S1 <= min(L, win_start + win_len).  Every product with n is taken in int64.
 * Row w of out [n_windows][c_max] (elements of the format) holds the resampler's outputs k in [K0, K1), K0 = ceil(n * S0 / o),
 * K1 = ceil(n * S1 / o): nout[w] = K1 - K0 values (nout: HOST int32 [n_windows] or NULL, written before the call returns); the entries
 * from there up to c_max are written as zero.  The cores of an utterance partition [0, L), so its chunks partition
 * [0, ceil(n * L / o)) = [0, ttsamd_resample_out_len(L)): nothing is emitted twice or dropped.
 * Value: out[f * n + p] = sum_{j < J} taps[p][j] * xz[f * o + j - width], xz = the utterance, read from the row at index - win_start
 * and zero outside [0, L); over j ascending as ONE fp32 fma chain from +0.f over all J taps, the chain of ttsamd_resample_forward's
 * general kernel: a chunk holds the bits of the whole-utterance call on the same samples.
 * Checked on the host (TTSAMD_EINVAL with a message, nothing launched, nout untouched): 1 <= n_windows <= TTSAMD_STREAM_MAX_WINDOWS;
 * the inequalities above; 1 <= win_len <= hop * w_max; nout[w] <= c_max; format in 0..3; wave and out 4-byte aligned; and the window
 * holds every in-utterance sample its outputs read: with f0 = K0 / n and f1 = (K1 - 1) / n, the interval
 * [max(0, f0 * o - width), min(L, f1 * o - width + J)) lies inside [win_start, win_start + win_len).  The kernel reads nothing of the
 * row outside that interval: the rest may hold anything.
 * format 0: fp32.  1: little-endian int16 PCM, s = clip(rint(x * 32767), -32768, 32767), fp32 product, ties to even, NaN -> 0
 * (ttsamd_stream_emit's format 1).  2: G.711 mu-law, one byte from s: a = s >> 2 (arithmetic), neg = a < 0,
 * m = min((neg ? -a : a) + 33, 8191), e = floor(log2(m)) - 5, byte = ~(neg << 7 | e << 4 | ((m >> (e + 1)) & 15)) & 0xff.
 * 3: G.711 A-law, one byte from s: a = s >> 3, pos = a >= 0, a = pos ? a : ~a, seg = a < 32 ? 0 : floor(log2(a)) - 4,
 * mant = seg < 2 ? (a >> 1) & 15 : (a >> seg) & 15, byte = (pos << 7 | seg << 4 | mant) ^ 0x55.  (tests/golden/g711.npz holds both
 * for every int16 value.) */
int32_t ttsamd_stream_emit_resampled(void* resample_handle, const float* wave, int32_t n_windows, int32_t w_max, int32_t hop,
                                     const int32_t* win_start /* host */, const int32_t* win_len /* host */,
                                     const int32_t* utt_len /* host */, const int32_t* core_start /* host */,
                                     const int32_t* core_end /* host */, int32_t c_max, int32_t format, void* out,
                                     int32_t* nout /* host, out, may be NULL */, void* stream);
/* Vocos in the stream (csrc/vocos.hip).  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.
 * The receptive field of a Vocos handle in mel frames per side, from its own num_layers and padding mode.  The backbone is the embed
 * conv (k = 7) and num_layers ConvNeXt blocks whose only mixing along time is a depthwise conv (k = 7), all zero-padded; LayerNorm, the
 * pointwise convs and head.out are per frame: 3 + 3 * num_layers frames per side (27 for 8 layers).  The ISTFT adds the frames whose
 * 1024-sample segments overlap a frame of samples.  Sample m = 256 c + j (0 <= j < 256) of frame c sums the frames t with
 * 0 <= m + pad - 256 t < 1024.  "same" (pad 384): 256 (c - t) + j + 384 in [0, 1024) holds for t = c - 2 (j < 128) ... c + 2
 * (j >= 128): frames c - 2 ... c + 2.  "center" (pad 512): 256 (c - t) + j + 512 in [0, 1024) holds for t = c - 1 ... c + 2, for no
 * j at t = c - 2.  So left / right = 3 + 3 * num_layers + (2, 2) for "same", + (1, 2) for "center": 29 / 29 for '22k', 28 / 29 for
 * '24k'.  With these halos the float64 oracle's window core equals its whole-utterance wave exactly; one frame less on either side
 * does not (2e-10 ... 1e-9 with the synthetic weights).  The spectral bias subtraction is per frame and adds nothing. */
int32_t ttsamd_vocos_halo_frames(void* handle, int32_t* left /* host, out */, int32_t* right /* host, out */);
/* The vocoder call of one streaming step.  mel [n_windows][input_channels][w_max] and lens int64 [n_windows] (device) are what
 * ttsamd_stream_gather writes; wave [n_windows][256 * w_max] is what both emit entries read.  need_start / need_len: HOST int32
 * [n_windows], read during the call and passed on as launch arguments (no staging copy, no host synchronisation): the FRAMES of window w
 * whose samples the caller will read, 0 <= need_start, 1 <= need_len, need_start + need_len <= lens[w] <= w_max.  denoise_rows: device
 * float [n_windows] or NULL (every row at 0); with it bias_vec is needed.
 * The backbone and head.out run over the whole windows as in ttsamd_vocos_forward_rows.  The head behind them runs only where the
 * needed samples can see it: the spectrum (with the row's denoise strength) and one 1024-point inverse FFT for the frames
 * [need_start - r_l, need_start + need_len + 2) within [0, lens[w]), r_l = 2 for "same" and 1 for "center" (the derivation above); the
 * overlap-add with the envelope for the samples [256 * need_start, 256 * (need_start + need_len)) within [0, n_out(lens[w])), n_out(L)
 * = 256 L for "same" and 256 (L - 1) for "center".  Those samples have the BITS of ttsamd_vocos_forward_rows on the same batch (the same
 * frames, summed in the same order); every other element of wave is NOT written.
 * ttsamd_vocos_workspace_bytes(handle, n_windows, w_max) is enough workspace (less: TTSAMD_ENOMEM).  Checked on the host
 * (TTSAMD_EINVAL with a message, nothing launched): NULL handle, mel, lens, wave or descriptor arrays; 1 <= n_windows <=
 * TTSAMD_STREAM_MAX_WINDOWS; w_max >= 1; 0 <= need_start, 1 <= need_len, need_start + need_len <= w_max; denoise_rows without
 * bias_vec.  lens[w] lives on the device and is not read back: the kernels clip both ranges to it, as stated above. */
int32_t ttsamd_vocos_forward_windows(void* handle, const float* mel, const int64_t* lens, int32_t n_windows, int32_t w_max,
                                     const int32_t* need_start /* host */, const int32_t* need_len /* host */,
                                     const float* denoise_rows /* device, may be NULL = 0 */, const float* bias_vec, float* wave,
                                     void* workspace, int64_t workspace_bytes, void* stream);
/* Backbone and head of a Vocos handle apart (csrc/vocos.hip).  New symbols only, added WITHOUT a bump: TTSAMD_ABI_VERSION stays 8.
 * ttsamd_vocos_features: mel and lens as for ttsamd_vocos_forward -> out [batch][1026][t_max], what head.out returns: rows 0 .. 512 the
 * log-magnitudes, rows 513 .. 1025 the phases, without the padding rows of the library's own buffer; frames t >= lens[b] are written
 * as zero.  The launches are those of ttsamd_vocos_forward up to the spectrum, so the values have its bits.
 * ttsamd_vocos_head: feats [batch][1026][t_max] in that layout -> wave [batch][256 * t_max] as ttsamd_vocos_forward_rows writes it:
 * mag = clamp(exp(log-magnitude) - denoise_rows[b] * bias_vec, 0, 100), times (cos, sin)(phase), one 1024-point inverse FFT per frame
 * t < lens[b], overlap-add with the handle's trimming ("same" / "center", ttsamd_vocos_set_padding); samples at or past a row's end are
 * not written, and "center" with t_max = 1 writes nothing.  denoise_rows: device float [batch] or NULL (no subtraction; a row at 0 has
 * the same bits); with it bias_vec is needed.  ttsamd_vocos_head(ttsamd_vocos_features(mel)) has the bits of ttsamd_vocos_forward_rows(mel).
 * ttsamd_vocos_workspace_bytes(handle, batch, t_max) is enough workspace for either (less: TTSAMD_ENOMEM). */
int32_t ttsamd_vocos_features(void* handle, const float* mel, const int64_t* lens, int32_t batch, int32_t t_max, float* out,
                              void* workspace, int64_t workspace_bytes, void* stream);
int32_t ttsamd_vocos_head(void* handle, const float* feats, const int64_t* lens, int32_t batch, int32_t t_max,
                          const float* denoise_rows /* device, may be NULL = 0 */, const float* bias_vec, float* wave, void* workspace,
                          int64_t workspace_bytes, void* stream);
/* The encoder alone, for finished waves: wave [batch][wave_stride] fp32 -> out [batch][out_stride] elements of format 1 (int16), 2 or 3
 * (one byte) as above.  nsamples: device int64 [batch], clamped to [0, wave_stride], or NULL for the full stride; samples
 * [0, nsamples[b]) of row b are converted, the entries behind them up to min(wave_stride, out_stride) are written as zero.  wave and
 * out 4-byte aligned, 1 <= batch <= 65535.  Nothing is read back to the host. */
int32_t ttsamd_wave_encode(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t format, void* out,
                           int64_t out_stride, void* stream);

/* ---- output levelling (csrc/loudness.hip): ITU-R BS.1770-4 integrated loudness and peak per row of a ragged mono batch, and one
 * gain per row towards a target.  wave [batch][wave_stride] fp32; nsamples: device int64 [batch], clamped to [0, wave_stride];
 * nothing at or past nsamples[b] is read or written, and nothing is read back to the host.
 *
 * K-weighting at sample_rate fs (8000 <= fs <= 192000): two biquads by the bilinear transform, in float64.  Stage 1 (shelf):
 * f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G / 20),
 * Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2, b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0],
 * a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0].  Stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773,
 * b = [1, -2, 1], a as in stage 1 with this stage's K and Q.  (At 48 kHz: the standard's table to its 14 decimals.)
 * y = stage 2 of stage 1 of the row from a zero state, in float64.  step = (fs + 5) / 10 samples (integer division: fs / 10 rounded,
 * a half upwards), block = 4 step.  A row of n >= block samples has J = (n - block) / step + 1 blocks, z_j = mean of y^2 over
 * [j step, j step + block); a row of 0 < n < block samples has the one block z_0 = mean of y^2 over its n samples (the standard
 * leaves such rows undefined); n = 0 has none.  l_j = -0.691 + 10 log10 z_j; absolute gate l_j > -70;
 * Gamma = -0.691 + 10 log10(mean of the z_j that pass it) - 10; L = -0.691 + 10 log10(mean of the z_j with l_j > -70 and
 * l_j > Gamma), -inf when no block passes the absolute gate.  peak = max |x| over the row, exact.
 * The filter runs as a scan: a row is cut into segments of S samples (S = the largest divisor of step that is <= 64), each segment's
 * zero-state response ends in a state that a second launch carries along the row with the 4 x 4 transition matrix of one segment
 * (built on the host with the coefficients), a third launch filters every segment again from its true state and sums y^2.  Four
 * launches whatever the lengths; every reduction has a fixed order that depends on the row's own length only, so row b of a batch
 * has the bits the row has alone. */
/* HOST out[10] float64: b1[0..2], a1[1..2], b2[0..2], a2[1..2]; TTSAMD_EINVAL outside 8000..192000.  Needs no GPU. */
int32_t ttsamd_loudness_coefficients(int32_t sample_rate, double* out);
/* bytes of workspace ttsamd_loudness_measure needs for this batch, stride and rate; -1: refused (batch < 1, a negative stride or
 * one of 2^40 and more, a rate outside 8000..192000) */
int64_t ttsamd_loudness_workspace_bytes(int32_t batch, int64_t wave_stride, int32_t sample_rate);
/* loudness: device float64 [batch] (LUFS, -inf for a silent or empty row); peak: device fp32 [batch].  1 <= batch <= 65535.
 * TTSAMD_EINVAL (nothing launched): a NULL pointer, batch < 1, a rate out of range, a workspace smaller than
 * ttsamd_loudness_workspace_bytes. */
int32_t ttsamd_loudness_measure(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t sample_rate,
                                double* loudness, float* peak, void* workspace, int64_t workspace_bytes, void* stream);
/* One launch: every row's gain from its loudness and peak (what ttsamd_loudness_measure wrote) and its mode and target (device int32 /
 * fp32 [batch], as ttsamd_denoise_rows takes its strengths), applied in place to samples [0, nsamples[b]); gain_out: device fp32 [batch].
 * mode 0: the row is not written, gain 1.  mode 1 (peak): x <- fl32(fl32(x / peak) * target) (numpy's float32 `x / m * 0.99`,
 * ttsamd_trim_apply's convention), gain_out = fl32(target / peak); peak == 0: not written, gain 1.  mode 2 (loudness, target in LUFS):
 * g = 10^((target - L) / 20) in float64; if peak g > ceiling, g = ceiling / peak (a cap on the gain, no limiter); g is rounded once
 * to fp32 (and taken one fp32 step down if fl32(peak g) > ceiling, so that the levelled peak never exceeds the ceiling) and
 * x <- fl32(x g); L not finite or peak == 0: not written, gain 1.
 * TTSAMD_EINVAL (nothing launched): a NULL pointer, batch < 1, a ceiling that is not in (0, 1].  The modes live on the device and are
 * not read back: the callers check them on the host before the upload (ttsamd.engine.LoudnessEngine.level refuses a mode outside
 * 0 .. 2 there), and the kernel leaves a row whose device value is outside 0 .. 2 as mode 0 does. */
int32_t ttsamd_wave_level(float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* mode,
                          const float* target, float ceiling, const double* loudness, const float* peak, float* gain_out, void* stream);

/* ---- look-ahead limiter (csrc/limiter.hip): a row gain and a gain-reduction curve, so that a LUFS target is reached where the cap of
 * ttsamd_wave_level stops short of it, and so that a fixed gain can be applied inside a stream.  wave [batch][wave_stride] fp32, in
 * place; nsamples: device int64 [batch], clamped to [0, wave_stride]; nothing at or past nsamples[b] is read or written and nothing is
 * read back to the host.  The curve is computed in Q30 integers (Q = 2^30): minimum and integer sum are exact and order-free, so a
 * row alone, a row of a ragged batch and a row cut into windows that carry the reach below leave with the same bits.
 * Per row, with n samples x, the row gain g (fp32), the ceiling c, attack A and hold R in samples (0 <= A <= R, A <= 1024, R <= 4096):
 *   u[i] = fl32(x[i] g);  d[i] = |u[i]|;  q[i] = Q if not d[i] > c, else floor((double)c / (double)d[i] 2^30) (a float64 division);
 *   m[i] = min q[j] over j in [i - R, i + A] within [0, n);
 *   s[i] = floor(sum over k = -A .. A of m[clamp(i + k, 0, n - 1)] / (2A + 1)) in int64;
 *   y[i] = (float)((double)u[i] (double)s[i] 2^-30)  (the product rounded to float64, then to fp32).
 * Every m term of s[i] has a window that contains i (A <= R), so s[i] <= q[i] and |y[i]| <= c holds exactly.  Where no sample within
 * reach exceeds the ceiling, y[i] = u[i] bit for bit.  One sample over the ceiling at j lowers the gain on [j - 2A, j + R + A], fully on
 * [j, j + R - A], with linear ramps.  y[i] depends on x over [i - A - R, i + 2A] only: the limiter's reach.  A NaN passes through
 * (q = Q), an infinity gives q = 0; memory-safe and unspecified beyond that.
 * Two launches: the q plane to the workspace, then blocks that own tiles of 2048 samples stage q for the tile plus reach in LDS, take the
 * sliding minimum by doubling and the box sum in int64, and write y. */
/* bytes of workspace ttsamd_wave_limit needs; -1: refused (batch < 1, a negative stride or one of 2^40 and more) */
int64_t ttsamd_wave_limit_workspace_bytes(int32_t batch, int64_t wave_stride);
/* mode: device int32 [batch], target: device fp32 [batch].  mode 0: the row is not written, gain 1.  mode 2 (target in LUFS):
 * g = fl32(min(10^((target - L) / 20), max_gain)) in float64 with L = loudness[b] (device float64 [batch], what
 * ttsamd_loudness_measure wrote) and NO cap from the peak; L not finite, or loudness NULL: not written, gain 1.  mode 3 (target is a gain
 * in dB, the stream's mode): g = fl32(min(10^(target / 20), max_gain)).  Any other device value is treated as mode 0 (the callers
 * check the modes on the host before the upload).  max_gain is linear, finite and > 0.  gain_out: device fp32 [batch];
 * reduction_out: device int32 [batch] = min over i of s[i]: Q where nothing was limited, and for a row that is empty or not written.
 * TTSAMD_EINVAL (nothing launched): a NULL pointer other than loudness, batch outside 1 .. 65535, a ceiling that is not in (0, 1], a
 * max_gain that is not finite and > 0, attack / hold outside the limits above, a workspace smaller than
 * ttsamd_wave_limit_workspace_bytes. */
int32_t ttsamd_wave_limit(float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* mode,
                          const float* target, float ceiling, float max_gain, int32_t attack, int32_t hold, const double* loudness,
                          float* gain_out, int32_t* reduction_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- true peak (csrc/true_peak.hpp, csrc/loudness.hip, csrc/limiter.hip): the peak of the 4x oversampled row, and the levelling and
 * the limiter against it.  New symbols only, added WITHOUT a bump.  Specified by the arithmetic below (the interpolator is the
 * project's own resampler table, not the FIR of ITU-R BS.1770-4 Annex 2; the EBU Tech 3341 true-peak signals read within that
 * document's +0.2 / -0.4 dB); parity with libebur128 / pyloudnorm is not pinned.
 * Interpolator: the resampler's formula above with o = 1, n = 4, lowpass_filter_width = 12, rolloff = 1.0: W = width = 12, J = 25 and,
 * in float64, t = clamp((j - 12) - p / 4, -12, 12), h[p][j] = sinc(t) cos^2(t pi / 24), rounded once to fp32 (in ttsamd/resample.py's
 * order of operations: the table is ttsamd.resample.resample_taps(1, 4, 12, 1.0)).  Only the phases p = 1, 2, 3 are used: phase 0 is
 * the sample itself, not a filtered copy.  The library builds the table on the host (ttsamd_true_peak_taps returns it) and hands it to
 * its kernels as an argument.  For a row x of n samples, xz = the row, zero outside [0, n):
 *   v[i][p] = sum over j = 0 .. 24 ascending of (double)h[p][j] (double)xz[i + j - 12], 0 <= i < n, a float64 accumulator from +0.0.
 * The product of two fp32 values is exact in float64, so fma and multiply-then-add give the same bits, and a numpy loop over j
 * reproduces the kernel bit for bit (an fp32 chain would not).
 * True peak: TP = max(max_i |x[i]|, max_{i, p} |v[i][p]|) in float64: the 4n positions i + p / 4 of a 4x resample, the tail behind the
 * last sample included, nothing before sample 0.  Returned as fp32 rounded UPWARD (the smallest fp32 >= TP), so that a ceiling
 * computed from it is never too lax; an empty row gives 0.  A maximum is order-free: row b of a batch has the bits the row has alone.
 * Level with a true-peak cap: ttsamd_wave_level with the true-peak array as its `peak`.  With H = max_p sum_j |h[p][j]| (from the
 * table), the levelled row y = fl32(x g) of mode 2 has TP(y) <= ceiling (1 + H 2^-24) up to the rounding of the gain itself: each
 * y[i] is within 2^-24 |x[i] g| of x[i] g, and the interpolator passes these errors with a gain of at most H.  (Strictly:
 * fl32(TP g) <= ceiling leaves TP g up to 2^-24 ceiling above the ceiling, so the proven bound is ceiling (1 + (H + 1) 2^-24
 * (1 + 2^-24)); mode 1 rounds twice, fl32(fl32(x / TP) target), and has target (1 + 2 H 2^-24 (1 + 2^-24)).  Both worst cases need
 * every rounding error under the 25 taps at its limit and with the taps' signs; the tests hold real rows to the first bound.)
 * Limiter with a true-peak detector: ttsamd_wave_limit's arithmetic literally (u, q, m, s, y, Q30) except for the detector d, which is
 * float64: with v computed from u as above (u zero outside the row),
 *   d[i] = max(|u[i]|, max_p |v[i][p]|, max_p |v[i - 1][p]|), the last term omitted for i = 0;
 *   q[i] = Q if not d[i] > (double)c, else floor((double)c / d[i] 2^30).
 * An inter-sample point between i and i + 1 pulls the gain down at both neighbours.  d[i] >= |u[i]|, so |y[i]| <= c still holds
 * exactly.  The reach grows by W + 1 = 13 on each side: y[i] depends on x over [i - A - R - 13, i + 2A + 13] only.  The true peak of y
 * is NOT bounded exactly by c: the gain curve varies across the 25 taps.  The overshoot is a measured number, not
 * a guarantee.
 * ttsamd_true_peak: two launches whatever the lengths (the result is zeroed, then blocks that own tiles of 2048 samples stage the tile
 * and 12 samples to either side in LDS, run the 3 chains per sample in registers and end in one unsigned integer atomic max per block:
 * non-negative IEEE floats order as their bit patterns).  The 4x signal is never written to memory. */
/* HOST out[3][25] float64: h[p][j] for p = 1, 2, 3 (each the widened fp32 value).  TTSAMD_EINVAL for NULL.  Needs no GPU. */
int32_t ttsamd_true_peak_taps(double* out);
/* true_peak: device fp32 [batch].  Nothing at or past nsamples[b] is read; nothing is read back to the host.
 * TTSAMD_EINVAL (nothing launched): a NULL pointer, batch outside 1 .. 65535, a negative stride or one of 2^40 and more. */
int32_t ttsamd_true_peak(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, float* true_peak, void* stream);
/* ttsamd_wave_limit with the detector above: the same arguments, modes, outputs, limits, TTSAMD_EINVAL rules and workspace
 * (ttsamd_wave_limit_workspace_bytes); two launches, the second is ttsamd_wave_limit's own. */
int32_t ttsamd_wave_limit_true_peak(float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* mode,
                                    const float* target, float ceiling, float max_gain, int32_t attack, int32_t hold,
                                    const double* loudness, float* gain_out, int32_t* reduction_out, void* workspace,
                                    int64_t workspace_bytes, void* stream);

/* ---- loudness meter (csrc/loudness.hip): EBU R 128 / Tech 3341 / 3342 momentary and short-term loudness, their maxima and the
 * loudness range, per row of a ragged mono batch and inside a stream.  New symbols only, added WITHOUT a bump.  Specified by the
 * arithmetic below; parity with libebur128 is left unpinned: libebur128 takes its short-term blocks for the range at another hop
 * (one block per second, here one per step of 100 ms), so the two populations of blocks, and with them the percentiles, differ.
 * Everything is float64.  With y, step, block, S (the segment) and Q = step / S of the output levelling above, for a row of n samples:
 *   step energies   u[i] = the sum of the Q segment sums of y^2 of step i, ascending, 0 <= i < U = n / step;
 *   momentary       z[j] = (((u[j] + u[j+1]) + u[j+2]) + u[j+3]) / block, 0 <= j < J: exactly the block energies of
 *                   ttsamd_loudness_measure, the short-row rule included (0 < n < block: J = 1, z[0] = mean of y^2 over the n samples;
 *                   n = 0: J = 0); M[j] = -0.691 + 10 log10 z[j];
 *   integrated loudness and peak: those of ttsamd_loudness_measure, bit for bit;
 *   short-term      JS = U - 29 values when U >= 30, else none; s[j] = (u[j] + .. + u[j+29]) / (30 step), summed ascending from 0;
 *                   S[j] = -0.691 + 10 log10 s[j].  The hop is one step, the overlap 2.9 s (Tech 3342 asks for at least 2 s);
 *   maxima          max_momentary = max_j M[j], max_short_term = max_j S[j]; -inf when there is no value;
 *   loudness range  keep the S[j] > -70; Gamma = -0.691 + 10 log10(mean of their s[j]) - 20; keep the S[j] > Gamma; with the k
 *                   survivors sorted ascending as v, LRA = v[((k - 1) 95 + 50) / 100] - v[((k - 1) 10 + 50) / 100] (integer
 *                   divisions: round((k - 1) p)); 0 when k = 0.
 * The three filter launches of ttsamd_loudness_measure, then ONE launch with a block per row: four launches whatever the lengths.
 * The percentiles are taken by rank counting (the rank of a survivor is the number of survivors below it, ties by index; the keys go
 * through LDS in tiles), so there is no cap on the length of a row.  Every sum has a fixed order that depends on the row's own length
 * only (the mean for Gamma: strided partial sums and an LDS tree, as the gates of the integrated loudness): row b of a batch has
 * the bits it has alone.  No atomics. */
/* bytes of workspace ttsamd_loudness_meter needs; -1: refused as ttsamd_loudness_workspace_bytes refuses */
int64_t ttsamd_loudness_meter_workspace_bytes(int32_t batch, int64_t wave_stride, int32_t sample_rate);
/* wave, nsamples, batch, sample_rate as ttsamd_loudness_measure.  Device outputs: loudness float64 [batch], peak fp32 [batch],
 * loudness_range, max_momentary, max_short_term float64 [batch], counts int64 [batch][2] = (J, JS).  momentary
 * [batch][momentary_stride] and short_term [batch][short_term_stride] float64 may be NULL; a stride is at least the J / JS of a row of
 * wave_stride samples, and entries at and past a row's own count are not written.  Nothing is read back to the host.
 * TTSAMD_EINVAL (nothing launched): a NULL pointer other than the two series, batch outside 1 .. 65535, a rate out of range, a series
 * stride too small, a workspace smaller than ttsamd_loudness_meter_workspace_bytes. */
int32_t ttsamd_loudness_meter(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t sample_rate,
                              double* loudness, float* peak, double* loudness_range, double* max_momentary, double* max_short_term,
                              int64_t* counts, double* momentary, int64_t momentary_stride, double* short_term, int64_t short_term_stride,
                              void* workspace, int64_t workspace_bytes, void* stream);
/* Stream meter: a device-resident state of `slots` slots, each a stream of at most max_samples samples at sample_rate; every call on a
 * state names the same three numbers.  A slot holds the four filter state doubles behind its last whole segment, the samples of the
 * unfinished segment (fewer than S), the sum of the finished segments of the unfinished step, the step energies u so far, the running
 * peak and a status word.  `slot`: device int32 [rows], one slot per row, no slot twice in a call; a row whose slot does not exist is
 * left out (push: its three readings are -inf; result: status 2).
 * push: chunks [rows][chunk_stride] fp32, nsamples device int64 [rows] clamped to [0, chunk_stride], any length.  Four launches: the
 * three filter launches run the row "unfinished segment, then the chunk" from the slot's filter state (the segments of a stream lie
 * on the stream's own grid whatever the chunking), the fourth takes the whole segments in: segment sums are added to the unfinished
 * step in order, a finished step goes to u.  Then per row: momentary = M of the last four steps and short_term = S of the last
 * thirty (-inf before there are four / thirty), integrated = both gates over all blocks so far (-inf before the first block: the
 * short-row rule is applied by result only).  A push that would take a slot beyond max_samples takes nothing in and sets bit 0 of
 * the slot's status; the readings are those of the samples so far.  A stream's values depend on its own samples and chunking only,
 * not on which other slots share the call.  Against the whole-wave entry the sums have the same order, but the filter state in front
 * of a segment comes through scans that start anew at every push: the results agree within 1e-9 LU, not bit for bit; the peak exactly.
 * result: loudness, loudness_range, max_momentary, max_short_term (float64 [rows]), peak (fp32 [rows]), counts (int64 [rows][2]) as
 * the whole-wave entry defines them over the samples so far (the short-row rule included), status int32 [rows].  One launch; the slot
 * is not changed.  reset: the slots named start again at zero samples (a new state is reset before its first push).
 * TTSAMD_EINVAL (nothing launched): a NULL pointer, slots or rows outside 1 .. 65535, max_samples outside 1 .. 2^40 - 1, a rate out
 * of range, a state smaller than ttsamd_meter_state_bytes, a workspace smaller than ttsamd_meter_push_workspace_bytes.
 * Nothing is read back to the host. */
int64_t ttsamd_meter_state_bytes(int32_t slots, int64_t max_samples, int32_t sample_rate);               /* -1: refused */
int64_t ttsamd_meter_push_workspace_bytes(int32_t rows, int64_t chunk_stride, int32_t sample_rate);      /* -1: refused */
int32_t ttsamd_meter_reset(void* state, int64_t state_bytes, int32_t slots, int64_t max_samples, int32_t sample_rate, const int32_t* slot,
                           int32_t rows, void* stream);
int32_t ttsamd_meter_push(void* state, int64_t state_bytes, int32_t slots, int64_t max_samples, int32_t sample_rate, const float* chunks,
                          int64_t chunk_stride, const int64_t* nsamples, const int32_t* slot, int32_t rows, double* momentary,
                          double* short_term, double* integrated, void* workspace, int64_t workspace_bytes, void* stream);
int32_t ttsamd_meter_result(void* state, int64_t state_bytes, int32_t slots, int64_t max_samples, int32_t sample_rate, const int32_t* slot,
                            int32_t rows, double* loudness, double* loudness_range, double* max_momentary, double* max_short_term, float* peak,
                            int64_t* counts, int32_t* status, void* stream);

/* ---- wave-against-wave scores (csrc/wavescore.hip): STOI / ESTOI at 10 kHz, SI-SDR / SNR and a log-spectral distance between the rows
 * of two ragged mono batches that are sample-aligned (copy synthesis, a precision mode against fp32, a delivery format against the float
 * wave; free-running synthesis is NOT aligned with a recording and has no meaningful score here).  Both waves are [batch][wave_stride]
 * fp32 and share nsamples: device int64 [batch], clamped to [0, wave_stride].  Nothing at or past nsamples[b] is read into a result and
 * nothing is read back to the host.  All arithmetic after the fp32 samples are loaded is float64: window products, the transforms
 * (radix-4 Stockham passes in LDS, with one radix-2 pass at 512 points; twiddles from a float64 table the block builds in LDS), powers, band sums and every statistic.  No
 * floating-point atomics and a fixed order in every reduction, which depends on the row's own length only: row b of a batch has the
 * bits of the call on row b alone, and two runs give the same bits.  1 <= batch <= 65535.
 * The scores are specified by the arithmetic below; parity with a release of pystoi (or any other package) is not pinned.
 *
 * STOI / ESTOI.  x = ref[b][0:n] (the clean signal), y = deg[b][0:n], both ALREADY at 10 000 Hz (ttsamd.engine.WaveScoreEngine resamples
 * with the project's own resampler, which is not pystoi's).  EPS = 2^-52, w = numpy.hanning(258)[1:-1] (256 points), hop 128, N = 30.
 *  1. F = (n - 256) / 128 + 1 frames for n >= 256, else 0; xf[f] = w * x[128 f : 128 f + 256], yf likewise.
 *  2. Silent frames go, decided on the clean signal: e[f] = 20 log10(sqrt(sum xf[f]^2) + EPS); frame f is kept when
 *     max_f e - 40 - e[f] < 0.  K kept frames, in order; both signals are rebuilt by overlap-add of their kept frames at hop 128
 *     (length 128 (K - 1) + 256; formed on the fly from the two kept frames that overlap a position).
 *  3. The rebuilt signals are framed again with w at hop 128 (K frames), zero-padded to 512 and transformed; P[k] = |X[k]|^2,
 *     tob[j] = sqrt(sum_{k = lo[j]}^{hi[j] - 1} P[k]) for the fifteen third-octave bands lo = 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69,
 *     87, 109, 138, 174 and hi = 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219 (the bins nearest to
 *     150 * 2^((2 j -/+ 1) / 6) Hz on the grid k * 10000 / 512).
 *  4. K < 30 (F = 0 included): score = 1e-5, the conventional "too short" value.
 *  5. For m = 30 .. K the segment is X_m = tob_x[:, m - 30 : m] (15 x 30), Y_m likewise; M = K - 29 segments.
 *  6. extended == 0 (STOI), per segment and band j: c = ||X_m[j]|| / (||Y_m[j]|| + EPS), Y' = min(c Y_m[j], X_m[j] (1 + 10^(15 / 20)));
 *     both rows are centred over the 30 frames and divided by (norm + EPS); score = the sum over m, j and t of the products / (15 M).
 *  7. extended != 0 (ESTOI), per segment: every row of X_m is centred over time and divided by (norm + EPS), then every column is
 *     centred over the bands and divided by (norm + EPS); the same for Y_m; score = sum over m of sum(Xn * Yn) / 30 / M.
 * An all-zero pair follows the arithmetic as written (every frame is kept, the score is 0).
 * score: device float64 [batch]; frames: device int32 [batch][2] = (F, K); tob_ref / tob_deg: device float64 [batch][15][f_max] or
 * NULL: the band magnitudes of step 3 for frames < min(K, f_max), zero from frame K on.  Three launches whatever the lengths. */
/* bytes of workspace ttsamd_stoi needs; -1: refused (batch < 1, a negative wave_stride or one of 2^31 and more) */
int64_t ttsamd_stoi_workspace_bytes(int32_t batch, int64_t wave_stride);
/* TTSAMD_EINVAL (nothing launched): a NULL pointer other than tob_ref / tob_deg, a batch or stride ttsamd_stoi_workspace_bytes refuses,
 * f_max < 0, a workspace smaller than ttsamd_stoi_workspace_bytes. */
int32_t ttsamd_stoi(const float* ref, const float* deg, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t extended,
                    double* score, int32_t* frames, double* tob_ref, double* tob_deg, int32_t f_max, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* SI-SDR and SNR of est against ref over n = nsamples[b] samples; out: device float64 [batch][2].  zero_mean != 0: both rows are
 * centred first (means in float64 over n, a pass of its own).  alpha = <est, ref> / <ref, ref>;
 * out[b][0] = 10 log10(sum (alpha ref)^2 / sum (alpha ref - est)^2), out[b][1] = 10 log10(sum ref^2 / sum (ref - est)^2).
 * IEEE results are kept as they fall: +inf for identical rows, NaN for n = 0, NaN (SI-SDR) for an all-zero reference.
 * One launch, one block per row: sample i is added by thread i mod 256 in ascending order and the block sum is a fixed tree
 * (ttsamd_dtw_aligned_eval's scheme).  TTSAMD_EINVAL: a NULL pointer, batch < 1, wave_stride < 0. */
int32_t ttsamd_wave_sdr(const float* ref, const float* est, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t zero_mean,
                        double* out, void* stream);
/* Log-spectral distance; out: device float64 [batch][2] = (lsd in dB, frames).  Frames of 1024 samples every 256, no padding:
 * F = (n - 1024) / 256 + 1, or 0 below 1024 samples; the periodic Hann window of the mel analysis (0.5 - 0.5 cos(2 pi i / 1024));
 * 1024-point transforms (the template of the 512-point one), P[k] = |X[k]|^2 for k = 0 .. 512, L[k] = 10 log10(max(P[k], 1e-10));
 * lsd = mean_f sqrt(mean_k (L_ref[k] - L_est[k])^2), NaN for F = 0.  One launch, one block per row, frames in order.
 * TTSAMD_EINVAL: a NULL pointer, batch < 1, wave_stride < 0. */
int32_t ttsamd_log_spectral_distance(const float* ref, const float* est, int64_t wave_stride, const int64_t* nsamples, int32_t batch,
                                     double* out, void* stream);

/* ---- multi-resolution STFT distance (csrc/mrstft.hip): the spectral convergence and the log-magnitude distance of Parallel WaveGAN's
 * loss, per resolution, between the rows of two sample-aligned ragged mono batches, with the conventions of the block above: both waves
 * [batch][wave_stride] fp32, nsamples device int64 [batch] clamped to [0, wave_stride], nothing at or past nsamples[b] read into a
 * result, nothing read back to the host, float64 after the fp32 samples are loaded (window products, the transforms: the template of
 * the block above at 512, 1024 and 2048 points, magnitudes, logarithms, every sum), no floating-point atomics and a fixed order in
 * every reduction that depends on the row's own length only: row b of a batch has the bits of the call on row b alone, and two runs
 * give the same bits.  1 <= batch <= 65535, 0 <= wave_stride < 2^31.
 * Specified by the arithmetic below; the framing is torch.stft(center=True, pad_mode='reflect')'s, parity with auraloss or with
 * Parallel WaveGAN's batch-wide sums is not pinned (there the sums run over a padded batch; here over the row's own frames only).
 *
 * n_res resolutions, 1 <= n_res <= 8, each (N = n_fft[r], H = hop[r], W = win[r]) with N in {512, 1024, 2048}, 1 <= W <= N, H >= 1
 * (HOST arrays).  For row b with n = nsamples[b] samples, for ref and for est:
 *  1. Window: w[i] = 0.5 - 0.5 cos(2 pi i / W) for i < W (periodic Hann), placed at offset (N - W) / 2 (rounded down) inside a frame of
 *     N, zero elsewhere.
 *  2. Reflect padding by P = N / 2 on both sides: padded index p maps to j = p - P, j < 0 -> -j, j >= n -> 2 (n - 1) - j.  This needs
 *     n > P: for a row with n <= P this resolution gives NaN for both numbers and 0 frames.
 *  3. F = 1 + n / H frames (rounded down); frame f is padded[f H : f H + N] * w, X[f][k] its N-point DFT for k = 0 .. N / 2.
 *  4. S[f][k] = sqrt(max(re^2 + im^2, 1e-7)).
 *  5. Spectral convergence: sc = sqrt(sum_{f,k} (S_ref - S_est)^2) / sqrt(sum_{f,k} S_ref^2).
 *  6. Log-magnitude distance: mag = sum_{f,k} |ln S_ref - ln S_est| / (F (N / 2 + 1)).
 * An identical pair gives exactly (0, 0): the two signals go through the same transform one after the other.
 * out: device float64 [batch][n_res][2] = (sc, mag); frames: device int32 [batch][n_res] = F.
 * n_res + 1 launches whatever the lengths: per resolution a block of N / 4 threads per 16 consecutive frames of a row writes its three
 * partial sums to the workspace (a thread adds the terms of its bins frame after frame; the block sums its threads by a butterfly over
 * the lanes of each wave, then the waves in ascending order); the last launch adds a row's partial sums in ascending order. */
/* bytes of workspace ttsamd_mr_stft needs; -1: refused (batch outside 1 .. 65535, wave_stride negative or so long that a resolution has
 * 2^31 frames or more, n_res outside 1 .. 8, a NULL array, a resolution outside the ranges above) */
int64_t ttsamd_mr_stft_workspace_bytes(int32_t batch, int64_t wave_stride, const int32_t* n_fft, const int32_t* hop, const int32_t* win,
                                       int32_t n_res);
/* TTSAMD_EINVAL (nothing launched, out and frames untouched): a NULL pointer, anything ttsamd_mr_stft_workspace_bytes refuses, a
 * workspace smaller than ttsamd_mr_stft_workspace_bytes. */
int32_t ttsamd_mr_stft(const float* ref, const float* est, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* n_fft,
                       const int32_t* hop, const int32_t* win, int32_t n_res, double* out, int32_t* frames, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ---- Griffin-Lim (csrc/griffinlim.hip): a linear magnitude -> wave without a vocoder, and the mel inversion in front of it.
 * n_fft = win = 1024, hop 256, the periodic Hann window of the mel analysis; the two framings of ttsamd_melspec_create, so that the mel
 * analysis of the result sees the frames that were given:
 *   framing 0 (same):   reflect padding 384 per side, T frames <-> n = 256 T samples,        T >= 2
 *   framing 1 (center): reflect padding 512 per side, T frames <-> n = 256 (T - 1) samples,  T >= 4   (torch.stft / istft, center=True)
 * Specified by its arithmetic, which is torchaudio.functional.griffinlim's for a linear magnitude (power 1):
 *   c = momentum / (1 + momentum);  angles = init;  tprev = 0
 *   n_iter times:  inv = istft(mag * angles);  rebuilt = stft(inv);  a = rebuilt - c * tprev (momentum != 0);
 *                  angles = a / (|a| + 1e-16);  tprev = rebuilt
 *   wave = istft(mag * angles)
 * istft: inverse real transform of each frame (the imaginary parts of bins 0 and 512 are dropped), times the window, overlap-add over
 * 256 (T - 1) + 1024 padded samples, divided by the sum of the squared windows of the frames that exist at that sample, cropped by the
 * padding.  stft: reflect padding at the row's own ends (j < 0 -> -j, j >= n -> 2 (n - 1) - j), frame t = padded[256 t : 256 t + 1024]
 * times the window.  In the center framing frame 0 is even about its middle, so its spectrum is real: the imaginary part of its
 * `rebuilt`, rounding noise only, is dropped.  The center framing is pinned against torch.stft / torch.istft; parity with a torchaudio release is not (the random
 * initial phase is the hash below).
 * mag: device fp32 [batch][513][t_max]; frames: device int32 [batch], clamped to [0, t_max]; a row below the framing's minimum is an empty
 * row (device data cannot be refused): a wave of zeros, inconsistency NaN.  Nothing at or past a row's frame count is read.
 * init 0: zero phase (angles = 1).  init 1: angle(t, k) = 2 pi (h >> 8) 2^-24 with
 *   h = fmix32(fmix32(seed_lo + 0x9E3779B9 (513 t + k)) ^ seed_hi)   (uint32 arithmetic, fmix32 = murmur3's finaliser)
 * under the row's 64-bit seed: seed_rows[b] (device uint64 [batch]) or, with seed_rows NULL, `seed` for every row -- a row's audio depends
 * on neither its batch nor its position.  init 2: angles = phase (which must not be NULL), used as they are.
 * phase: device complex64 [batch][t_max][513] or NULL; when not NULL it receives the final angles of the frames below the row's count
 * (the rest is not written): 1 + 1 iterations through `phase` are 2 iterations when momentum is 0 (tprev is not carried).
 * wave: device fp32 [batch][wave_stride], wave_stride >= the n of t_max; samples at or past the row's n are written as zero.
 * inconsistency: device float64 [batch] or NULL: || |rebuilt| - mag || / || mag || over the row's frames and bins, from the last
 * iteration's `rebuilt` (no extra transform; |rebuilt| - mag in fp32, the two sums in float64: per-block partial sums in a fixed order,
 * then one fixed-order sum per row); NaN for n_iter = 0.
 * fp32 arithmetic.  n_iter + 3 launches whatever the batch and the lengths; between two iterations the windowed inverse frames
 * [batch][t_max][1024] cross HBM (a ping-pong pair in the workspace) and, with momentum != 0, tprev [batch][t_max][513] complex: no
 * other spectrum matrix exists.  Row b of a batch has the bits of the call on row b alone; two runs give the same bits. */
/* bytes of workspace ttsamd_griffinlim needs; -1: refused (batch outside 1 .. 65535, t_max outside 1 .. 2^22) */
int64_t ttsamd_griffinlim_workspace_bytes(int32_t batch, int32_t t_max, float momentum);
/* TTSAMD_EINVAL (nothing launched): a NULL mag / frames / wave / workspace, a framing other than 0 / 1, t_max below the framing's
 * minimum (the message names it), n_iter < 0, momentum outside [0, 1), init outside 0 .. 2 or init 2 without phase, a wave_stride
 * below the n of t_max or of 2^31 - 1024 and more, a workspace smaller than ttsamd_griffinlim_workspace_bytes. */
int32_t ttsamd_griffinlim(const float* mag, const int32_t* frames, int32_t batch, int32_t t_max, int32_t framing, int32_t n_iter,
                          float momentum, int32_t init, const uint64_t* seed_rows, uint64_t seed, void* phase, float* wave,
                          int64_t wave_stride, double* inconsistency, void* workspace, int64_t workspace_bytes, void* stream);
/* Mel inversion by the pseudo-inverse of the filterbank: mag[b][f][t] = max(sum_m pinv[f][m] e(mel[b][m][t]), floor) for t < frames[b],
 * 0 from there on; e = exp when log_input != 0 (the natural log of a clamped mel, as the HiFi-GAN analysis writes it), the identity
 * otherwise.  mel: device fp32 [batch][n_mels][t_max], 1 <= n_mels <= 128; pinv: device fp32 [513][n_mels] (computed once by the caller,
 * in float64); mag: device fp32 [batch][513][t_max].  One launch, fp32, m ascending. */
int32_t ttsamd_mel_to_linear(const float* mel, const int32_t* frames, int32_t batch, int32_t n_mels, int32_t t_max, const float* pinv,
                             int32_t log_input, float floor, float* mag, void* stream);

/* Timing hooks for bench.py (roofline of the dominant kernel): when enabled, hifigan
 * forward brackets its ResBlock conv launches with HIP events on the launch stream. */
int32_t ttsamd_profile_enable(int32_t on);
/* Fills: [0] = conv-kernel ms (length of the union of the timed sections' intervals), [1] = number of conv launches,
 * [2] = number of timed sections (event pairs: a single launch, or one fork..join group of concurrent launches) */
int32_t ttsamd_profile_read(double* out3);

#ifdef __cplusplus
}
#endif
#endif /* TTSAMD_H */
