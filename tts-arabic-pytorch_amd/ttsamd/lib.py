"""ctypes binding of libttsamd.so — one Python function per symbol of include/ttsamd.h."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# TTSAMD_LIB: another build of the SAME sources (A/B of two builds: tools/fp_digest.py); the product path never sets it
LIB_PATH = os.environ.get('TTSAMD_LIB') or os.path.join(_HERE, 'lib', 'libttsamd.so')


class TtsAmdError(RuntimeError):
    pass


class Tensor(C.Structure):
    _fields_ = [('name', C.c_char_p), ('data', C.POINTER(C.c_float)), ('ndim', C.c_int32),
                ('shape', C.c_int64 * 4)]


class HifiGanCfg(C.Structure):
    _fields_ = [('num_mels', C.c_int32), ('upsample_initial_channel', C.c_int32), ('n_ups', C.c_int32),
                ('upsample_rates', C.c_int32 * 8), ('upsample_kernel_sizes', C.c_int32 * 8),
                ('n_kernels', C.c_int32), ('resblock_kernel_sizes', C.c_int32 * 8),
                ('n_dilations', C.c_int32), ('resblock_dilations', (C.c_int32 * 8) * 8), ('resblock', C.c_int32)]


class FastPitchCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        'n_mel_channels', 'n_symbols', 'padding_idx', 'd_model',
        'in_fft_n_layers', 'in_fft_n_heads', 'in_fft_d_head', 'in_fft_kernel', 'in_fft_filter',
        'out_fft_n_layers', 'out_fft_n_heads', 'out_fft_d_head', 'out_fft_kernel', 'out_fft_filter',
        'dur_kernel', 'dur_filter', 'dur_n_layers',
        'pitch_kernel', 'pitch_filter', 'pitch_n_layers', 'pitch_emb_kernel',
        'energy_conditioning', 'energy_kernel', 'energy_filter', 'energy_n_layers', 'energy_emb_kernel',
        'n_speakers')] + [('speaker_emb_weight', C.c_float)]


class Tacotron2Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        'n_symbol', 'num_speakers', 'speaker_embedding_dim', 'symbol_embedding_dim', 'encoder_embedding_dim',
        'encoder_n_convolution', 'encoder_kernel_size', 'n_mels', 'prenet_dim', 'attention_rnn_dim',
        'decoder_rnn_dim', 'attention_hidden_dim', 'attention_location_n_filter',
        'attention_location_kernel_size', 'postnet_n_convolution', 'postnet_kernel_size',
        'postnet_embedding_dim')] + [('gate_threshold', C.c_float), ('decoder_early_stopping', C.c_int32)]


class TaggerCfg(C.Structure):
    _fields_ = [('n_vocab', C.c_int32), ('emb_dim', C.c_int32), ('n_lstm', C.c_int32), ('lstm_hidden', C.c_int32 * 4),
                ('hard_sigmoid', C.c_int32), ('bn_after_lstm0', C.c_int32), ('bn_eps', C.c_float),
                ('n_dense', C.c_int32), ('dense_dim', C.c_int32 * 4)]


class AlignerCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('n_mel', 'd_text', 'n_att', 'n_symbols', 'padding_idx')]


class PyinCfg(C.Structure):
    _fields_ = [('sample_rate', C.c_int32), ('frame_length', C.c_int32), ('win_length', C.c_int32), ('hop_length', C.c_int32),
                ('fmin', C.c_double), ('fmax', C.c_double), ('n_thresholds', C.c_int32), ('beta_a', C.c_int32), ('beta_b', C.c_int32),
                ('boltzmann', C.c_double), ('resolution', C.c_double), ('max_transition_rate', C.c_double),
                ('switch_prob', C.c_double), ('no_trough_prob', C.c_double), ('pad_mode', C.c_int32)]


# every symbol include/ttsamd.h declares: name -> (restype, argtypes)
_P, _I32, _I64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
SYMBOLS = {
    'ttsamd_last_error': (C.c_char_p, []),
    'ttsamd_version': (_I32, []),
    'ttsamd_set_option': (_I32, [C.c_char_p, C.c_char_p]),
    'ttsamd_get_option': (_I32, [C.c_char_p, C.c_char_p, _I32]),
    'ttsamd_option_name': (C.c_char_p, [_I32]),
    'ttsamd_options_check': (_I32, []),
    'ttsamd_device_ok': (_I32, []),
    'ttsamd_hifigan_create': (_I32, [C.POINTER(Tensor), _I32, C.POINTER(HifiGanCfg), C.POINTER(_P)]),
    'ttsamd_hifigan_destroy': (_I32, [_P]),
    'ttsamd_hifigan_workspace_bytes': (_I64, [_P, _I32, _I32]),
    'ttsamd_hifigan_forward': (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _I64, _P]),
    # streaming synthesis (csrc/stream.hip): the window descriptors are HOST int32 arrays
    'ttsamd_hifigan_halo_frames': (_I32, [_P, C.POINTER(_I32), C.POINTER(_I32)]),
    'ttsamd_denoiser_halo_frames': (_I32, []),
    'ttsamd_stream_gather': (_I32, [_P, _I32, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _P, _P]),
    'ttsamd_stream_emit': (_I32, [_P, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P]),
    # ... resampled and encoded (format 0 fp32, 1 int16 PCM, 2 mu-law, 3 A-law): handle (or NULL), wave, W, w_max, hop, five HOST int32
    # arrays in utterance samples, c_max, format, out, nout (HOST int32, out), stream
    'ttsamd_stream_emit_resampled': (_I32, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P]),
    # Vocos in the stream (csrc/vocos.hip): handle, mel, lens, W, w_max, need_start / need_len (HOST int32), denoise_rows, bias_vec, wave,
    # workspace, bytes, stream
    'ttsamd_vocos_halo_frames': (_I32, [_P, C.POINTER(_I32), C.POINTER(_I32)]),
    'ttsamd_vocos_forward_windows': (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _I64, _P]),
    'ttsamd_wave_encode': (_I32, [_P, _I64, _P, _I32, _I32, _P, _I64, _P]),
    'ttsamd_fastpitch_create': (_I32, [C.POINTER(Tensor), _I32, C.POINTER(FastPitchCfg), C.POINTER(_P)]),
    'ttsamd_fastpitch_destroy': (_I32, [_P]),
    'ttsamd_fastpitch_encode_workspace_bytes': (_I64, [_P, _I32, _I32]),
    'ttsamd_fastpitch_decode_workspace_bytes': (_I64, [_P, _I32, _I32]),
    'ttsamd_fastpitch_encode': (_I32, [_P, _P, _I32, _I32, _I32, _F, _P, _P, _P, _F, _F, _F,
                                       _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    'ttsamd_length_regulate': (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'ttsamd_fastpitch_decode': (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _I64, _P]),
    'ttsamd_fastpitch_set_batch_mode': (_I32, [_P, _I32]),
    # ... with per-row speaker / pace / pitch_mul / pitch_add arrays (device, each may be NULL) and flags (bit 0: rows as if alone)
    'ttsamd_fastpitch_encode_rows': (_I32, [_P, _P, _I32, _I32, _I32, _F, _P, _P, _P, _F, _F, _F,
                                            _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _I32, _P]),
    'ttsamd_fastpitch_decode_rows': (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _I64, _I32, _P]),
    'ttsamd_denoiser_create': (_I32, [C.POINTER(_P)]),
    'ttsamd_denoiser_destroy': (_I32, [_P]),
    'ttsamd_denoiser_workspace_bytes': (_I64, [_I32, _I32]),
    'ttsamd_denoiser_bias_spec': (_I32, [_P, _P, _P, _I32, _P, _P, _I64, _P]),
    'ttsamd_denoise': (_I32, [_P, _P, _I64, _P, _I32, _I32, _P, _F, _P, _I64, _P]),
    'ttsamd_denoise_rows': (_I32, [_P, _P, _I64, _P, _I32, _I32, _P, _P, _P, _I64, _P]),
    'ttsamd_vocos_create': (_I32, [C.POINTER(Tensor), _I32, _I32, _I32, _I32, _I32, C.POINTER(_P)]),
    'ttsamd_vocos_destroy': (_I32, [_P]),
    'ttsamd_vocos_workspace_bytes': (_I64, [_P, _I32, _I32]),
    'ttsamd_vocos_bias_vec': (_I32, [_P, _P, _P, _I64, _P]),
    'ttsamd_vocos_forward': (_I32, [_P, _P, _P, _I32, _I32, _F, _P, _P, _P, _I64, _P]),
    'ttsamd_vocos_forward_rows': (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    'ttsamd_vocos_set_padding': (_I32, [_P, _I32]),
    # backbone and head apart (csrc/vocos.hip): handle, mel, lens, B, T, out [B][1026][T], ws, ws_bytes, stream /
    # handle, feats, lens, B, T, denoise_rows or NULL, bias_vec, wave, ws, ws_bytes, stream
    'ttsamd_vocos_features': (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _I64, _P]),
    'ttsamd_vocos_head': (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    'ttsamd_melspec_create': (_I32, [_P, _I32, _I32, _I32, _I32, _I32, _F, C.POINTER(_P)]),
    'ttsamd_melspec_destroy': (_I32, [_P]),
    'ttsamd_melspec_forward': (_I32, [_P, _P, _I64, _P, _I32, _I32, _P, _P, _P]),
    'ttsamd_cepstral_series': (_I32, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _P, _P, _P]),
    'ttsamd_cepstral_series_from_power': (_I32, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, C.c_double, C.c_double, _F, _P, _P]),
    'ttsamd_series_summary': (_I32, [_P, _P, _I32, _I32, _I32, _P, _P, _P]),
    'ttsamd_dtw_workspace_bytes': (_I64, [_I32, _I32, _I32, _I32]),
    'ttsamd_dtw': (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    'ttsamd_dtw_aligned_mae': (_I32, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    'ttsamd_mel_cepstrum': (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    'ttsamd_dtw_aligned_eval': (_I32, [_P, _P, _I32, _I32, _P, _P, _I32, _P, _P, _I32, _I32, _I32, _P, _P, C.c_double, _P, _P]),
    'ttsamd_aligner_create': (_I32, [C.POINTER(Tensor), _I32, C.POINTER(AlignerCfg), C.POINTER(_P)]),
    'ttsamd_aligner_destroy': (_I32, [_P]),
    'ttsamd_aligner_workspace_bytes': (_I64, [_P, _I32, _I32, _I32]),
    'ttsamd_aligner_forward': (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _P]),
    'ttsamd_mas_workspace_bytes': (_I64, [_I32, _I32, _I32]),
    'ttsamd_mas': (_I32, [_P, _I32, _P, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _P]),
    'ttsamd_average_pitch': (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    'ttsamd_attn_prior': (_I32, [_P, _P, _I32, _I32, _I32, _I32, C.c_double, _P, _P]),
    'ttsamd_attn_prior_tables': (_I32, [_I32, _P]),
    'ttsamd_attn_ctc_loss_workspace_bytes': (_I64, [_I32, _I32, _I32]),
    'ttsamd_attn_ctc_loss': (_I32, [_P, _P, _P, _I32, _I32, _I32, C.c_double, _P, _P, _I64, _P]),
    'ttsamd_attn_bin_loss': (_I32, [_P, _P, _I32, _I32, _I32, C.c_double, _P, _P, _P]),
    'ttsamd_pyin_tables': (_I32, [C.POINTER(PyinCfg), _P, _P, _P, _P, _P, _P, _P]),
    'ttsamd_pyin_create': (_I32, [C.POINTER(PyinCfg), C.POINTER(_P)]),
    'ttsamd_pyin_destroy': (_I32, [_P]),
    'ttsamd_pyin_workspace_bytes': (_I64, [_P, _I32, _I32]),
    'ttsamd_pyin_obs_offsets': (_I32, [_P, _I32, _I32, _P]),
    'ttsamd_pyin_forward': (_I32, [_P, _P, _I64, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _I64, _P]),
    'ttsamd_resample_create': (_I32, [_P, _I32, _I32, _I32, C.POINTER(_P)]),
    'ttsamd_resample_destroy': (_I32, [_P]),
    'ttsamd_resample_out_len': (_I64, [_P, _I64]),
    'ttsamd_resample_mfma_eligible': (_I32, [_P]),
    'ttsamd_resample_forward': (_I32, [_P, _P, _I64, _P, _I32, _P, _I64, _P, _I32, _P]),
    'ttsamd_trim_workspace_bytes': (_I64, [_I32, _I64, _I32]),
    'ttsamd_trim_bounds': (_I32, [_P, _I64, _P, _I32, _F, _I32, _I32, _F, _P, _P, _P, _I64, _P]),
    'ttsamd_trim_apply': (_I32, [_P, _I64, _P, _P, _F, _I64, _I32, _P, _I64, _P, _P]),
    'ttsamd_frames_compact': (_I32, [_P, _P, _P, _I32, _I32, _I32, _I32, _F, _P, _P, _P, _P]),
    # paragraph join (csrc/join.hip): wave, wave_stride, nsamples, bounds (or NULL), gap, B, fade, F, keep, lead, out, out_stride, segs
    # (int64 [B][4]), total (int64 [1]), stream
    'ttsamd_wave_join': (_I32, [_P, _I64, _P, _P, _P, _I32, _P, _I32, _I64, _I64, _P, _I64, _P, _P, _P]),
    # token and word spans (csrc/timing.hip): reps, reps_stride, n_tokens (or NULL), B, L, groups (int32 [B][G][2] or NULL), n_groups (or
    # NULL), G, hop, map (int64 [B][5] or NULL), tok (int64 [B][L][2]), grp (int64 [B][G][2] or NULL), stream
    'ttsamd_token_spans': (_I32, [_P, _I64, _P, _I32, _I32, _P, _P, _I32, _I64, _P, _P, _P, _P]),
    # output levelling (csrc/loudness.hip): the coefficients go to a HOST float64 [10] and need no GPU
    'ttsamd_loudness_coefficients': (_I32, [_I32, C.POINTER(C.c_double)]),
    'ttsamd_loudness_workspace_bytes': (_I64, [_I32, _I64, _I32]),
    'ttsamd_loudness_measure': (_I32, [_P, _I64, _P, _I32, _I32, _P, _P, _P, _I64, _P]),
    'ttsamd_wave_level': (_I32, [_P, _I64, _P, _I32, _P, _P, _F, _P, _P, _P, _P]),
    # look-ahead limiter (csrc/limiter.hip): gain fp32 [B] and reduction int32 [B] (Q30) on the device
    'ttsamd_wave_limit_workspace_bytes': (_I64, [_I32, _I64]),
    'ttsamd_wave_limit': (_I32, [_P, _I64, _P, _I32, _P, _P, _F, _F, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    # true peak (csrc/true_peak.hpp): the taps go to a HOST float64 [3][25] and need no GPU; true_peak fp32 [B] on the device
    'ttsamd_true_peak_taps': (_I32, [C.POINTER(C.c_double)]),
    'ttsamd_true_peak': (_I32, [_P, _I64, _P, _I32, _P, _P]),
    'ttsamd_wave_limit_true_peak': (_I32, [_P, _I64, _P, _I32, _P, _P, _F, _F, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    # loudness meter (csrc/loudness.hip): float64 results and series, counts int64 [B][2] on the device; the stream meter's state
    'ttsamd_loudness_meter_workspace_bytes': (_I64, [_I32, _I64, _I32]),
    'ttsamd_loudness_meter': (_I32, [_P, _I64, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _P]),
    'ttsamd_meter_state_bytes': (_I64, [_I32, _I64, _I32]),
    'ttsamd_meter_push_workspace_bytes': (_I64, [_I32, _I64, _I32]),
    'ttsamd_meter_reset': (_I32, [_P, _I64, _I32, _I64, _I32, _P, _I32, _P]),
    'ttsamd_meter_push': (_I32, [_P, _I64, _I32, _I64, _I32, _P, _I64, _P, _P, _I32, _P, _P, _P, _P, _I64, _P]),
    'ttsamd_meter_result': (_I32, [_P, _I64, _I32, _I64, _I32, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _P]),
    # wave-against-wave scores (csrc/wavescore.hip): float64 results, lengths int64 on the device
    'ttsamd_stoi_workspace_bytes': (_I64, [_I32, _I64]),
    'ttsamd_stoi': (_I32, [_P, _P, _I64, _P, _I32, _I32, _P, _P, _P, _P, _I32, _P, _I64, _P]),
    'ttsamd_wave_sdr': (_I32, [_P, _P, _I64, _P, _I32, _I32, _P, _P]),
    'ttsamd_log_spectral_distance': (_I32, [_P, _P, _I64, _P, _I32, _P, _P]),
    # multi-resolution STFT distance (csrc/mrstft.hip): the resolution arrays are HOST int32 [n_res]
    'ttsamd_mr_stft_workspace_bytes': (_I64, [_I32, _I64, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), _I32]),
    'ttsamd_mr_stft': (_I32, [_P, _P, _I64, _P, _I32, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), _I32, _P, _P, _P, _I64, _P]),
    # Griffin-Lim (csrc/griffinlim.hip): mag, frames (int32), B, t_max, framing, n_iter, momentum, init, seed_rows (uint64 [B] or NULL), seed,
    # phase (complex64 or NULL), wave, wave_stride, inconsistency (float64 [B] or NULL), workspace, bytes, stream
    'ttsamd_griffinlim_workspace_bytes': (_I64, [_I32, _I32, _F]),
    'ttsamd_griffinlim': (_I32, [_P, _P, _I32, _I32, _I32, _I32, _F, _I32, _P, C.c_uint64, _P, _P, _I64, _P, _P, _I64, _P]),
    'ttsamd_mel_to_linear': (_I32, [_P, _P, _I32, _I32, _I32, _P, _I32, _F, _P, _P]),
    'ttsamd_tacotron2_create': (_I32, [C.POINTER(Tensor), _I32, C.POINTER(Tacotron2Cfg), C.POINTER(_P)]),
    'ttsamd_tacotron2_destroy': (_I32, [_P]),
    'ttsamd_tacotron2_workspace_bytes': (_I64, [_P, _I32, _I32, _I32]),
    'ttsamd_tacotron2_infer': (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I64, _P, _P, _P, _P,
                                      C.POINTER(_I32), _P, _I64, _P]),
    # the same decode as a session of advances (csrc/tacotron2.hip); steps_done, ended and the row report are HOST int32
    'ttsamd_tacotron2_stream_bytes': (_I64, [_P, _I32, _I32, _I32, _I32]),
    'ttsamd_tacotron2_stream_begin': (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I64, _P, _I32, _P, _P, _P, _P, _I64,
                                             C.POINTER(_P), _P]),
    'ttsamd_tacotron2_stream_advance': (_I32, [_P, _I32, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), _P]),
    'ttsamd_tacotron2_stream_end': (_I32, [_P]),
    'ttsamd_tacotron2_postnet_halo_frames': (_I32, [_P, C.POINTER(_I32)]),
    'ttsamd_tacotron2_postnet_window_bytes': (_I64, [_P, _I32, _I32]),
    'ttsamd_tacotron2_postnet_window': (_I32, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I64, _P]),
    'ttsamd_tagger_create': (_I32, [C.POINTER(Tensor), _I32, C.POINTER(TaggerCfg), C.POINTER(_P)]),
    'ttsamd_tagger_destroy': (_I32, [_P]),
    'ttsamd_tagger_workspace_bytes': (_I64, [_P, _I32, _I32]),
    'ttsamd_tagger_forward': (_I32, [_P, _P, _I32, _I32, _P, _P, _I64, _P]),
    'ttsamd_conv1d_packed_floats': (_I64, [_I32, _I32, _I32]),
    'ttsamd_conv1d': (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P, _P, _P]),
    'ttsamd_conv1d_ex': (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _I32, _F, _P, _P, _P]),
    'ttsamd_conv1d_splitk': (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _I32, _F, _P, _P, _P, _I64, _P]),
    'ttsamd_conv_last_launch': (_I32, [C.POINTER(_I32), C.POINTER(_I32)]),
    'ttsamd_conv1d_route': (_I32, [_I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _I32, _I32, _I64, C.POINTER(_I32), C.POINTER(_I32)]),
    'ttsamd_convt_packed_floats': (_I64, [_I32, _I32, _I32]),
    'ttsamd_conv_transpose1d': (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F, _P, _P, _P]),
    'ttsamd_convt_wino_packed_floats': (_I64, [_I32, _I32, _I32]),
    'ttsamd_convt_wino_pack_weight': (_I32, [_P, _P, _I32, _I32, _I32, _P]),
    'ttsamd_resblock_pair_packed_floats': (_I64, [_I32, _I32, _I32]),
    'ttsamd_resblock_pair': (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _I32, _I32, _I32, _I32, _F, _F, _I32, _P, _I64, _P]),
    'ttsamd_resblock_pair_route': (_I32, [_I32, _I32, _I32, _I32, _I32] + [C.POINTER(_I32)] * 4 + [C.POINTER(C.c_char_p)]),
    'ttsamd_resblock2_packed_floats': (_I64, [_I32, _I32, _I32]),
    'ttsamd_resblock2': (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I32, _I32, _I32, _I32, _F, _F, _I32, _P, _I64, _P]),
    'ttsamd_set_precision': (_I32, [_I32]),
    'ttsamd_get_precision': (_I32, []),
    'ttsamd_dp_unique_id': (_I32, [_P]),
    'ttsamd_dp_init': (_I32, [_I32, _I32, _P, C.POINTER(_P)]),
    'ttsamd_dp_destroy': (_I32, [_P]),
    'ttsamd_dp_rank': (_I32, [_P]),
    'ttsamd_dp_world': (_I32, [_P]),
    'ttsamd_dp_broadcast': (_I32, [_P, _P, _I64, _I32, _P]),
    'ttsamd_dp_broadcast_weights': (_I32, [_P, _I32, _P, _I32, _P]),
    'ttsamd_dp_allgather': (_I32, [_P, _P, _P, _I64, _P]),
    'ttsamd_dp_pack_audio': (_I32, [_P, _I64, _P, _I32, _I64, _P, _P]),
    'ttsamd_dp_gather_audio': (_I32, [_P, _P, _P, C.POINTER(_I64), C.POINTER(_I64), _I32, _P]),
    'ttsamd_profile_enable': (_I32, [_I32]),
    'ttsamd_profile_read': (_I32, [C.POINTER(C.c_double)]),
}
# the bf16 octet engine's kernel-level entries, the same eight for both modes: ttsamd_bfo_* (plain bf16) and ttsamd_bfo3_* (split bf16)
_BFO = {
    'pack': (_I32, [_P, _I32, _I32, _I32, _F, _P, _P]),
    'unpack': (_I32, [_P, _I32, _I32, _I32, _F, _P, _P]),
    'weight_elems': (_I64, [_I32, _I32, _I32, _I32]),
    'pack_weight': (_I32, [_P, _I32, _I32, _I32, _I32, _P]),
    'conv1d': (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _F, _F, _P, _P, _P, _P]),
    'resblock_pair': (_I32, [_P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _F, _F, _F, _P, _P]),
    'resblock_chain': (_I32, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F, _F, _F, _F, _P, _P, _I32]),   # last: k
    'conv_post': (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I64, _P]),
}
for _prefix in ('bfo', 'bfo3'):
    for _name, (_res, _args) in _BFO.items():
        # the x3 chain entry takes no kernel size (k = 3)
        SYMBOLS[f'ttsamd_{_prefix}_{_name}'] = (_res, _args[:-1] if (_prefix, _name) == ('bfo3', 'resblock_chain') else _args)

_lib = None
ABI_VERSION = 8            # == TTSAMD_ABI_VERSION of include/ttsamd.h (struct layouts and argument meanings of this binding)


def load():
    """dlopen libttsamd.so (built by `make -C tts-arabic-pytorch_amd/csrc` or
    __graft_entry__.build()).  Fails loudly — there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TtsAmdError(f'{LIB_PATH} is missing: build it with `make -C tts-arabic-pytorch_amd/csrc` '
                          '(hipcc --offload-arch=gfx950); there is no CPU/PyTorch fallback')
    # torch bundles its own libamdhip64.so.7; it must be the first HIP runtime in the process
    # (two runtimes = "No HIP GPUs are available"), so pull it in before dlopen-ing ours, which then
    # binds to the already-loaded SONAME.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    got = lib.ttsamd_version()
    if got != ABI_VERSION:
        raise TtsAmdError(f'{LIB_PATH} was built from another revision of include/ttsamd.h (library ABI {got}, this binding '
                          f'{ABI_VERSION}): rebuild it with `make -C tts-arabic-pytorch_amd/csrc`')
    if lib.ttsamd_options_check() != 0:             # a malformed TTSAMD_<NAME> in the environment: loud, not ignored
        msg = lib.ttsamd_last_error()
        raise TtsAmdError(f'bad routing option in the environment: {msg.decode() if msg else "?"}')
    _lib = lib
    return lib


def set_option(name, value):
    """Routing option of the library (include/ttsamd.h: ttsamd_set_option): `name` with or without the TTSAMD_ prefix, `value` an int / str
    as the environment variable would hold it, None = back to the default.  Raises on an unknown name or a value out of range."""
    v = None if value is None else str(value).encode()
    check(load().ttsamd_set_option(name.encode(), v), f'set_option({name}={value})')


def get_option(name):
    """Current text of a routing option, None when unset (the default applies)."""
    buf = C.create_string_buffer(64)
    check(load().ttsamd_get_option(name.encode(), buf, 64), f'get_option({name})')
    return buf.value.decode() or None


def option_names():
    lib, out, i = load(), [], 0
    while True:
        n = lib.ttsamd_option_name(i)
        if not n:
            return out
        out.append(n.decode())
        i += 1


class options:
    """Context manager: set routing options for a block and restore what was there before.  `with options(TTSAMD_WINO=0): ...`"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            set_option(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            set_option(k, v)


def check(rc, what):
    if rc != 0:
        msg = load().ttsamd_last_error()
        raise TtsAmdError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')


def make_tensors(state_dict):
    """{name: np.float32 array or torch tensor} -> (ctypes array of Tensor, keep-alive list)."""
    import numpy as np
    keep, items = [], []
    for name, v in state_dict.items():
        if hasattr(v, 'detach'):
            if not v.is_floating_point():
                continue
            v = v.detach().cpu().float().numpy()
        a = np.ascontiguousarray(v, dtype=np.float32)
        if a.ndim > 4:
            continue
        t = Tensor()
        nb = name.encode()
        t.name = nb
        t.data = a.ctypes.data_as(C.POINTER(C.c_float))
        t.ndim = a.ndim
        for i, s in enumerate(a.shape):
            t.shape[i] = s
        keep += [a, nb]
        items.append(t)
    arr = (Tensor * len(items))(*items)
    return arr, keep
