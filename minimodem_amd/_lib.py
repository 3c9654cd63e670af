"""ctypes binding of libmifsk.so (the C ABI declared in include/fsk.h and
include/mifsk.h, and the extension headers under include/mifsk/).  The library is built in-tree by `minimodem_amd.build()` /
`__graft_entry__.build()`; if it is missing or cannot be loaded this module
raises -- there is no Python or CPU fallback for the signal path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIFSK_LIBRARY selects another build of the same library (e.g. libmifsk_prof.so)
LIB_PATH = os.environ.get("MIFSK_LIBRARY") or os.path.join(_HERE, "libmifsk.so")
MAX_BITS = 64


class ModemArgs(C.Structure):
    _fields_ = [
        ("baudmode", C.c_char_p),
        ("sample_rate", C.c_uint),
        ("mark_f", C.c_float),
        ("space_f", C.c_float),
        ("band_width", C.c_float),
        ("n_data_bits", C.c_int),
        ("baudot", C.c_int),
        ("nstartbits", C.c_int),
        ("nstopbits", C.c_float),
        ("invert_start_stop", C.c_int),
        ("inverted_freqs", C.c_int),
        ("msb_first", C.c_int),
        ("have_sync_byte", C.c_int),
        ("sync_byte", C.c_longlong),
        ("confidence_threshold", C.c_float),
        ("search_limit", C.c_float),
        ("binary_output", C.c_int),
        ("binary_raw_nbits", C.c_int),
        ("rx_one", C.c_int),
        ("auto_carrier_threshold", C.c_float),
    ]


class RxConfig(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_uint),
        ("data_rate", C.c_float),
        ("mark_f", C.c_float),
        ("space_f", C.c_float),
        ("band_width", C.c_float),
        ("n_data_bits", C.c_uint),
        ("nstartbits", C.c_int),
        ("nstopbits", C.c_float),
        ("invert_start_stop", C.c_int),
        ("msb_first", C.c_int),
        ("do_rx_sync", C.c_int),
        ("sync_byte", C.c_ulonglong),
        ("decoder", C.c_int),
        ("rx_one", C.c_int),
        ("confidence_threshold", C.c_float),
        ("search_limit", C.c_float),
        ("auto_carrier_threshold", C.c_float),
        ("autodetect_shift", C.c_int),
        ("inverted_freqs", C.c_int),
        ("fftsize", C.c_int),
        ("nbands", C.c_uint),
        ("b_mark", C.c_uint),
        ("b_space", C.c_uint),
        ("frame_n_bits", C.c_uint),
        ("nsamples_per_bit", C.c_float),
        ("nsamples_overscan", C.c_uint),
        ("frame_nsamples", C.c_uint),
        ("expect_n_bits", C.c_uint),
        ("expect_nsamples", C.c_uint),
        ("expect_data", C.c_char * (MAX_BITS + 4)),
        ("expect_sync", C.c_char * (MAX_BITS + 4)),
        ("samplebuf_size", C.c_uint),
        ("try_first", C.c_uint * 2),
        ("try_max", C.c_uint * 2),
        ("try_step", C.c_uint * 2),
        ("try_step_fine", C.c_uint * 2),
        ("find_samples_per_bit", C.c_float),
        ("bit_nsamples", C.c_uint),
        ("bit_offset", C.c_uint * MAX_BITS),
    ]

    def as_dict(self):
        out = {}
        for name, _t in self._fields_:
            v = getattr(self, name)
            if isinstance(v, bytes):
                v = v.decode()
            elif hasattr(v, "__len__"):
                v = list(v)
            out[name] = v
        return out


class Search(C.Structure):
    _fields_ = [
        ("sample_offset", C.c_uint64),
        ("navail", C.c_uint32),
        ("try_first", C.c_uint32),
        ("try_max", C.c_uint32),
        ("try_step", C.c_uint32),
        ("search_limit", C.c_float),
        ("use_sync_string", C.c_uint32),
    ]


class SearchResult(C.Structure):
    _fields_ = [
        ("bits", C.c_uint64),
        ("confidence", C.c_float),
        ("amplitude", C.c_float),
        ("frame_start", C.c_uint32),
        ("n_positions", C.c_uint32),
    ]


# what every io of a batch entry begins with: the rows (base, elements between them, per-row
# lengths or NULL, the length of every row then) and their number
ROWS_FIELDS = [("d_samples", C.c_void_p), ("stream_stride", C.c_size_t), ("d_nsamples", C.c_void_p),
               ("nsamples", C.c_uint32), ("nstreams", C.c_int)]


class DemodIO(C.Structure):
    _fields_ = ROWS_FIELDS + [
        ("d_bytes", C.c_void_p),
        ("d_nbytes", C.c_void_p),
        ("d_bits", C.c_void_p),
        ("d_frames", C.c_void_p),
        ("d_nframes", C.c_void_p),
        ("frames_cap", C.c_size_t),
        ("d_episodes", C.c_void_p),
        ("d_nepisodes", C.c_void_p),
        ("episodes_cap", C.c_size_t),
        ("d_status", C.c_void_p),
        ("d_counters", C.c_void_p),
        ("d_carrier_band", C.c_void_p),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]

class LaunchInfo(C.Structure):
    _fields_ = [
        ("kernel", C.c_char * 64),
        ("engine", C.c_uint32), ("workgroup_size", C.c_uint32),
        ("lds_bytes_per_workgroup", C.c_uint32), ("workgroups_per_cu", C.c_uint32),
        ("lattice_mode", C.c_uint32), ("frames_per_block", C.c_uint32),
        ("compute_units", C.c_uint32),
        ("chain_groups", C.c_uint32), ("chain_chunks", C.c_uint32),
    ]


class PipelineInfo(C.Structure):
    _fields_ = [("depth_requested", C.c_uint32), ("depth", C.c_uint32),
                ("hw_queues", C.c_uint32), ("output_sets", C.c_uint32)]


class GatherInfo(C.Structure):
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("device", C.c_int),
                ("slots", C.c_uint32), ("loopback", C.c_uint32), ("communicator", C.c_uint32)]


class SessionResult(C.Structure):
    _fields_ = [("nframes", C.c_uint32), ("nbytes", C.c_uint32), ("nepisodes", C.c_uint32),
                ("status", C.c_uint32), ("carrier_band", C.c_int32), ("finished", C.c_uint32),
                ("bits", C.c_void_p), ("bytes", C.c_void_p), ("frames", C.c_void_p),
                ("episodes", C.c_void_p), ("consumed", C.c_uint64)]


class SessionInfo(C.Structure):
    _fields_ = [("resident", C.c_uint32), ("feeds", C.c_uint32), ("row_capacity", C.c_uint64),
                ("device_bytes", C.c_uint64), ("h2d_bytes_last", C.c_uint64),
                ("h2d_bytes_total", C.c_uint64), ("reserved", C.c_uint64 * 2)]


SESSION_WANT_FRAMES = 0x1000
SESSION_RESIDENT = 0x2000
FEED_F32, FEED_S16 = 0, 1
GATHER_ID_BYTES = 128
GATHER_LOOPBACK = 1
WANT_BYTES, WANT_BITS, WANT_FRAMES, WANT_EPISODES = 1, 2, 4, 8
PIPELINE_NO_PRODUCER = C.c_void_p(-1)
IO_RING_EXACT = 1
IO_ENGINE_WORKGROUP = 2
# mifsk_selftest_corr routines (MIFSK_SELFTEST_CORR_*)
CORR_ROUTINES = {"lds_fixed": 0, "lds_fixed_halves": 1, "lds_stream": 2, "lds_stream_lean": 3,
                 "global_stream": 4, "global_tiled": 5, "slab_plain": 6, "skewed_stream": 7, "seg_group": 8}
SCAN_ROUTINES = {"asm": 0, "soft": 1, "track": 2}
IO_ENGINE_WAVE = 4
IO_HOST_S16 = 0x100
FILES_WANT_FRAMES = 0x1000


class HostStats(C.Structure):
    _fields_ = [("seconds_total", C.c_double), ("seconds_staging", C.c_double),
                ("bytes_h2d", C.c_uint64), ("bytes_d2h", C.c_uint64),
                ("chunks", C.c_uint32), ("streams", C.c_uint32),
                ("source_pinned", C.c_uint32), ("reserved", C.c_uint32)]


class FskPlan(C.Structure):
    """struct fsk_plan, include/fsk.h (layout of reference src/fsk.h:30-46)."""
    _fields_ = [
        ("sample_rate", C.c_float), ("f_mark", C.c_float), ("f_space", C.c_float),
        ("filter_bw", C.c_float), ("fftsize", C.c_int), ("nbands", C.c_uint),
        ("band_width", C.c_float), ("b_mark", C.c_uint), ("b_space", C.c_uint),
        ("fftplan", C.c_void_p), ("fftin", C.c_void_p), ("fftout", C.c_void_p),
    ]


class WavInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_uint), ("channels", C.c_uint), ("bits_per_sample", C.c_uint),
                ("is_float", C.c_int), ("data_offset", C.c_size_t), ("nframes", C.c_size_t)]


class ScanPlan(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("nseg", C.c_uint32), ("npass", C.c_uint32), ("nwin", C.c_uint32),
                ("span_hi", C.c_uint32), ("pass_len", C.c_uint32 * 2), ("pass_min", C.c_uint32 * 2),
                ("bound_c", C.c_float), ("seg_rel", C.c_uint32 * 128), ("seg_len", C.c_uint16 * 128),
                ("slot_seg", C.c_uint16 * 128), ("win_first", C.c_uint16 * 128),
                ("win_count", C.c_uint16 * 128), ("p_slot", C.c_uint32 * 128), ("p_win", C.c_uint32 * 128),
                ("p_slot_seg", C.c_uint8 * 128)]


class FileResult(C.Structure):
    _fields_ = [("error", C.c_int), ("info", WavInfo), ("cfg", C.POINTER(RxConfig)),
                ("nframes", C.c_uint32), ("nbytes", C.c_uint32), ("nepisodes", C.c_uint32),
                ("status", C.c_uint32), ("carrier_band", C.c_int32), ("reserved", C.c_uint32),
                ("bits", C.c_void_p), ("bytes", C.c_void_p), ("frames", C.c_void_p),
                ("episodes", C.c_void_p)]


class TimeSplit(C.Structure):
    _fields_ = [("chunk", C.c_uint64), ("warmup", C.c_uint64), ("chunks", C.c_uint32),
                ("flags", C.c_uint32)]


class TimeSplitStats(C.Structure):
    _fields_ = [("nsamples", C.c_uint64), ("chunk", C.c_uint64), ("warmup", C.c_uint64),
                ("lattice", C.c_uint64), ("samples_speculative", C.c_uint64),
                ("samples_rerun", C.c_uint64), ("nchunks", C.c_uint32), ("accepted", C.c_uint32),
                ("rerun", C.c_uint32), ("rounds", C.c_uint32)]


TIME_SPLIT_REJECT_ALL = 0x10000


class SoftbitsIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("kind", C.c_uint32), ("rxnoise", C.c_float),
                              ("d_origin", C.c_void_p), ("d_frames", C.c_void_p), ("d_nframes", C.c_void_p),
                              ("frames_cap", C.c_size_t), ("d_mag", C.c_void_p), ("d_rawbits", C.c_void_p)]


CARRIER_NONE, CARRIER_NO_WINDOW = -1, -2


class CarrierIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("kind", C.c_uint32), ("rxnoise", C.c_float),
                              ("first", C.c_uint64), ("window", C.c_uint32), ("hop", C.c_uint32), ("nwindows", C.c_uint32),
                              ("threshold", C.c_float), ("d_band", C.c_void_p), ("d_mag", C.c_void_p),
                              ("d_spectrum", C.c_void_p)]


CHANNEL_COMPLEX = 1


class ChannelParams(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("phase_steps", C.c_uint32), ("ntaps", C.c_uint32),
                ("taps", C.c_void_p), ("decim", C.c_uint32), ("nchannels", C.c_uint32), ("centres", C.c_void_p),
                ("out_centre", C.c_int32)]


class ChannelIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("d_rows", C.c_void_p),
                              ("out_stride", C.c_size_t), ("nout_cap", C.c_uint32), ("d_nout", C.c_void_p)]


MUX_COMPLEX = 1


class MuxParams(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("phase_steps", C.c_uint32), ("ntaps", C.c_uint32),
                ("taps", C.c_void_p), ("interp", C.c_uint32), ("nchannels", C.c_uint32), ("centres", C.c_void_p),
                ("in_centre", C.c_int32), ("gains", C.c_void_p)]


class MuxIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("d_out", C.c_void_p),
                              ("out_stride", C.c_size_t), ("nout_cap", C.c_uint32), ("d_nout", C.c_void_p)]


class ImpairIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("kind", C.c_uint32), ("out_kind", C.c_uint32),
                              ("d_out", C.c_void_p), ("out_stride", C.c_size_t), ("seed", C.c_uint64),
                              ("first_stream", C.c_uint64), ("first_sample", C.c_uint64), ("d_gain", C.c_void_p),
                              ("d_sigma", C.c_void_p), ("d_dc", C.c_void_p), ("gain", C.c_float), ("sigma", C.c_float),
                              ("dc", C.c_float), ("flags", C.c_uint32)]


class FmDemodIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("kind", C.c_uint32), ("flags", C.c_uint32),
                              ("d_out", C.c_void_p), ("out_stride", C.c_size_t), ("d_prev", C.c_void_p), ("d_last", C.c_void_p),
                              ("gain", C.c_float), ("reserved", C.c_uint32)]


class FmModIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("out_kind", C.c_uint32), ("flags", C.c_uint32),
                              ("d_out", C.c_void_p), ("out_stride", C.c_size_t), ("deviation", C.c_double), ("centre", C.c_double),
                              ("d_phase0", C.c_void_p), ("d_phase_out", C.c_void_p), ("amplitude", C.c_float),
                              ("reserved", C.c_uint32)]


# C struct name -> its mirror, for every struct of include/*.h that has one here (mifsk_frame, mifsk_episode
# and mifsk_stream_state are numpy dtypes only: DTYPES in __init__.py)
STRUCTS = {
    "fsk_plan": FskPlan, "mifsk_modem_args": ModemArgs, "mifsk_rx_config": RxConfig, "mifsk_search": Search,
    "mifsk_search_result": SearchResult, "mifsk_demod_io": DemodIO, "mifsk_pipeline_info": PipelineInfo,
    "mifsk_gather_info": GatherInfo, "mifsk_launch_info": LaunchInfo, "mifsk_scan_plan": ScanPlan,
    "mifsk_host_stats": HostStats, "mifsk_time_split": TimeSplit, "mifsk_time_split_stats": TimeSplitStats,
    "mifsk_session_result": SessionResult, "mifsk_session_info": SessionInfo, "mifsk_softbits_io": SoftbitsIO,
    "mifsk_carrier_io": CarrierIO, "mifsk_channel_params": ChannelParams, "mifsk_channel_io": ChannelIO,
    "mifsk_mux_params": MuxParams, "mifsk_mux_io": MuxIO, "mifsk_impair_io": ImpairIO,
    "mifsk_fm_demod_io": FmDemodIO, "mifsk_fm_mod_io": FmModIO, "mifsk_wav_info": WavInfo,
    "mifsk_file_result": FileResult,
}

_P = C.POINTER
_vp, _str, _int, _uint, _f32, _f64 = C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.c_float, C.c_double
_sz, _u32, _u64 = C.c_size_t, C.c_uint32, C.c_uint64
_cfg, _io, _split, _split_stats = _P(RxConfig), _P(DemodIO), _P(TimeSplit), _P(TimeSplitStats)

# every function include/*.h declares, in the headers' order: name -> (restype, argtypes); None: void
SIGNATURES = {
    # include/fsk.h
    "fsk_plan_new": (_P(FskPlan), [_f32, _f32, _f32, _f32]),
    "fsk_plan_destroy": (None, [_vp]),
    "fsk_find_frame": (_f32, [_vp, _vp, _uint, _uint, _uint, _uint, _f32, _str, _P(C.c_ulonglong), _P(_f32),
                              _P(_uint)]),
    "fsk_detect_carrier": (_int, [_vp, _vp, _uint, _f32]),
    "fsk_set_tones_by_bandshift": (None, [_vp, _uint, _int]),
    # include/mifsk.h: the configuration
    "mifsk_modem_args_default": (None, [_P(ModemArgs)]),
    "mifsk_rx_config_init": (_int, [_cfg, _P(ModemArgs)]),
    "mifsk_max_frames": (_sz, [_cfg, _sz]),
    "mifsk_stream_padding": (_sz, [_cfg]),
    # device context
    "mifsk_ctx_create": (_int, [_P(_vp), _int]),
    "mifsk_ctx_destroy": (None, [_vp]),
    "mifsk_ctx_device_name": (_str, [_vp]),
    "mifsk_abi_version": (_int, []),
    "mifsk_abi_sizeof": (_sz, [_str]),
    # diagnostics (declared with the device context)
    "mifsk_selftest_sqrt": (_int, [_vp, _u64, _u64, _P(_u64)]),
    "mifsk_selftest_rcp": (_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "mifsk_selftest_mag": (_int, [_vp, _vp, _vp, _f32, _u64, _vp, _vp, _vp, _vp]),
    "mifsk_selftest_confidence": (_int, [_vp, _int, _u32, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "mifsk_selftest_gauss": (_int, [_vp, _vp, _u64, _vp]),
    "mifsk_selftest_turn": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "mifsk_selftest_corr": (_int, [_vp, _cfg, _int, _int, _vp, _u32, _vp, _vp, _u32, _vp, _vp]),
    "mifsk_selftest_scan": (_int, [_vp, _int, _int, _vp, _vp, _vp, _vp, _u32, _vp, _vp]),
    "mifsk_selftest_wave_max": (_int, [_vp, _vp, _u32, _vp]),
    # N independent fsk_find_frame() problems; the whole-stream receive loop
    "mifsk_find_frame_batch": (_int, [_vp, _cfg, _vp, _vp, _vp, _int, _vp]),
    "mifsk_demod_batch": (_int, [_vp, _cfg, _io, _vp]),
    # several batches in flight
    "mifsk_pipeline_create": (_int, [_P(_vp), _int, _int]),
    "mifsk_pipeline_destroy": (None, [_vp]),
    "mifsk_pipeline_info_get": (_int, [_vp, _P(PipelineInfo)]),
    "mifsk_pipeline_outputs_alloc": (_int, [_vp, _int, _sz, _sz, _uint]),
    "mifsk_pipeline_outputs_get": (_int, [_vp, _u64, _io]),
    "mifsk_pipeline_submit": (_int, [_vp, _cfg, _io, _vp, _P(_u64)]),
    "mifsk_pipeline_next_ticket": (_u64, [_vp]),
    "mifsk_pipeline_wait": (_int, [_vp, _u64]),
    "mifsk_pipeline_join": (_int, [_vp, _u64, _vp]),
    "mifsk_pipeline_drain": (_int, [_vp]),
    "mifsk_pipeline_stream": (_vp, [_vp, _u64]),
    "mifsk_pipeline_ctx": (_vp, [_vp, _u64]),
    # one process per GPU: decoded bytes to one rank
    "mifsk_gather_unique_id": (_int, [_vp]),
    "mifsk_gather_create": (_int, [_P(_vp), _vp, _int, _int, _int, _int, _uint]),
    "mifsk_gather_destroy": (None, [_vp]),
    "mifsk_gather_info_get": (_int, [_vp, _P(GatherInfo)]),
    "mifsk_gather_start": (_int, [_vp, _vp, _sz, _vp, _int, _int, _P(_int), _vp, _P(_u64)]),
    "mifsk_gather_received": (_int, [_vp, _u64, _int, _P(_vp), _P(_vp), _P(_int), _P(_int)]),
    # what a batch would launch
    "mifsk_demod_plan": (_int, [_vp, _cfg, _int, _uint, _P(LaunchInfo)]),
    "mifsk_demod_plan_ex": (_int, [_vp, _cfg, _int, _u32, _uint, _P(LaunchInfo)]),
    "mifsk_scan_plan_get": (_int, [_cfg, _int, _P(ScanPlan)]),
    # streams that start in host memory
    "mifsk_demod_batch_host": (_int, [_vp, _cfg, _io]),
    "mifsk_demod_batch_host_ex": (_int, [_vp, _cfg, _io, _f32, _P(HostStats)]),
    "mifsk_host_alloc": (_vp, [_sz]),
    "mifsk_host_free": (None, [_vp]),
    "mifsk_max_episodes": (_sz, [_cfg, _sz]),
    # streams that arrive in pieces
    "mifsk_demod_slab": (_int, [_vp, _cfg, _io, _vp, _vp, _int, _vp]),
    "mifsk_ring_floats": (_sz, [_cfg]),
    "mifsk_demod_slab_ring": (_int, [_vp, _cfg, _io, _vp, _vp, _vp, _int, _vp]),
    # one long recording across the whole chip
    "mifsk_time_split_plan_get": (_int, [_cfg, _u64, _split, _split_stats]),
    "mifsk_demod_long": (_int, [_vp, _cfg, _vp, _u64, _split, _io, _split_stats, _vp]),
    "mifsk_time_split_plan_batch_get": (_int, [_cfg, _P(_u64), _int, _split, _split_stats]),
    "mifsk_demod_long_batch": (_int, [_vp, _cfg, _vp, _sz, _P(_u64), _int, _split, _io, _split_stats, _vp]),
    "mifsk_demod_long_batch_s16": (_int, [_vp, _cfg, _vp, _sz, _P(_u64), _int, _f32, _split, _io, _split_stats,
                                          _vp]),
    "mifsk_demod_long_batch_host": (_int, [_vp, _cfg, _P(_vp), _P(_u64), _int, _uint, _f32, _split, _io,
                                           _split_stats, _P(HostStats)]),
    # streams fed in pieces from host memory; the resident session
    "mifsk_session_create": (_int, [_P(_vp), _vp, _cfg, _int, _uint]),
    "mifsk_session_destroy": (None, [_vp]),
    "mifsk_session_feed": (_int, [_vp, _P(_vp), _P(_u32), _int]),
    "mifsk_session_get": (_P(SessionResult), [_vp, _int]),
    "mifsk_session_pending": (_sz, [_vp, _int]),
    "mifsk_session_feed_ex": (_int, [_vp, _P(_vp), _P(_u32), _uint, _f32, _int]),
    "mifsk_session_feed_device": (_int, [_vp, _vp, _sz, _P(_u32), _uint, _f32, _int, _vp]),
    "mifsk_session_info_get": (_int, [_vp, _P(SessionInfo)]),
    # soft bits; a batch of fsk_detect_carrier() problems
    "mifsk_frame_softbits": (_int, [_vp, _cfg, _P(SoftbitsIO), _vp]),
    "mifsk_detect_carrier_batch": (_int, [_vp, _cfg, _P(CarrierIO), _vp]),
    "mifsk_carrier_windows": (_u64, [_u64, _u64, _u32, _u32]),
    "mifsk_carrier_tones": (_int, [_cfg, _int, _P(_uint), _P(_uint), _P(_f32), _P(_f32)]),
    # channelizer
    "mifsk_channel_plan_create": (_int, [_vp, _P(ChannelParams), _P(_vp)]),
    "mifsk_channel_plan_destroy": (None, [_vp]),
    "mifsk_channelize_batch": (_int, [_vp, _P(ChannelIO), _vp]),
    "mifsk_channel_table": (_int, [_P(ChannelParams), _u32, _vp]),
    "mifsk_channel_taps": (_int, [_u32, _f64, _f64, _f64, _vp]),
    # multiplexer
    "mifsk_mux_plan_create": (_int, [_vp, _P(MuxParams), _P(_vp)]),
    "mifsk_mux_plan_destroy": (None, [_vp]),
    "mifsk_multiplex_batch": (_int, [_vp, _P(MuxIO), _vp]),
    "mifsk_mux_table": (_int, [_P(MuxParams), _vp]),
    # channel model
    "mifsk_impair_batch": (_int, [_vp, _P(ImpairIO), _vp]),
    "mifsk_impair_sigma": (_f32, [_f32, _f64]),
    # FM stage
    "mifsk_fm_demod_batch": (_int, [_vp, _P(FmDemodIO), _vp]),
    "mifsk_fm_gain": (_f32, [_f64, _f64]),
    "mifsk_fm_modulate_batch": (_int, [_vp, _P(FmModIO), _vp]),
    "mifsk_fm_step": (_f64, [_f64, _f64]),
    # several GPUs
    "mifsk_shard_range": (None, [_int, _int, _int, _P(_int), _P(_int)]),
    "mifsk_demod_batch_host_multi": (_int, [_P(_vp), _int, _cfg, _io]),
    # host post-pass: frame bits -> text
    "mifsk_databits_create": (_int, [_P(_vp), _int]),
    "mifsk_databits_destroy": (None, [_vp]),
    "mifsk_databits_reset": (None, [_vp]),
    "mifsk_databits_decode": (_uint, [_vp, _str, _uint, C.c_ulonglong, _uint]),
    "mifsk_databits_encode": (_uint, [_vp, _P(_uint), C.c_char]),
    "mifsk_stream_text": (_int, [_cfg, _vp, _u32, _vp, _u32, _uint, _str, _sz, _P(_sz), _str, _sz, _P(_sz)]),
    # input side: the step before the path
    "mifsk_wav_parse": (_int, [_str, _sz, _P(WavInfo)]),
    "mifsk_ingest_s16": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u32, _int, _f32, _vp]),
    "mifsk_ingest_rxnoise_f32": (_int, [_vp, _vp, _sz, _vp, _u32, _int, _f32, _vp]),
    # a list of audio files -> one batch
    "mifsk_demod_files": (_int, [_vp, _P(ModemArgs), _P(_str), _int, _f32, _uint, _P(_vp)]),
    "mifsk_demod_files_long": (_int, [_vp, _P(ModemArgs), _P(_str), _int, _f32, _uint, _split, _P(_vp)]),
    "mifsk_files_time_split": (_split_stats, [_vp, _int]),
    "mifsk_files_count": (_int, [_vp]),
    "mifsk_files_get": (_P(FileResult), [_vp, _int]),
    "mifsk_files_stats": (_P(HostStats), [_vp]),
    "mifsk_files_free": (None, [_vp]),
    # transmit side
    "mifsk_tx_synthesize": (C.c_long, [_cfg, _vp, _sz, _uint, _f32, _uint, _int, _vp, _sz]),
    "mifsk_tx_synthesize_batch": (_int, [_vp, _cfg, _vp, _sz, _vp, _u32, _int, _uint, _f32, _vp, _u32, _int, _vp,
                                         _sz, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)

# what the extension headers under include/mifsk/ declare, bound like SIGNATURES: additions that leave the
# ABI of include/*.h (its prototypes, structs and MIFSK_ABI_VERSION) as it is.  EXT_SIGNATURES is the first
# such header's table; EXTENSIONS below holds one per header, and load() binds them all.
EXT_SIGNATURES = {
    # include/mifsk/channel_iq.h
    "mifsk_channelize_iq_batch": (_int, [_vp, _P(ChannelIO), _vp]),
}
# one table per extension header, by the header's path under include/
EXTENSIONS = {
    "mifsk/channel_iq.h": EXT_SIGNATURES,
    "mifsk/mux_iq.h": {"mifsk_multiplex_iq_batch": (_int, [_vp, _P(MuxIO), _vp])},
}

# include/mifsk/channel_stream.h, the channelizer fed in pieces: a third extension header.  Its table is a name
# of its own (EXTENSIONS stays the two stateless entries' headers), which load() binds as well.
CHANNEL_STREAM_IQ = 1
STREAM_HEADER = "mifsk/channel_stream.h"
STREAM_SIGNATURES = {
    "mifsk_channel_stream_create": (_int, [_vp, _int, _P(_vp)]),
    "mifsk_channel_stream_destroy": (None, [_vp]),
    "mifsk_channel_stream_feed": (_int, [_vp, _P(ChannelIO), _u32, _vp]),
    "mifsk_channel_stream_seek": (_int, [_vp, _P(_u64), _vp]),
    "mifsk_channel_stream_seen": (_int, [_vp, _P(_u64), _vp]),
    "mifsk_channel_stream_outputs": (_u64, [_u32, _u32, _u64, _u64]),
}

# include/mifsk/mux_stream.h, the multiplexer fed in pieces: the fourth extension header, bound like the third
# from a table of its own (SIGNATURES, EXPORTS, EXT_SIGNATURES, EXTENSIONS and STREAM_SIGNATURES stay as they are).
MUX_STREAM_IQ = 1
MUX_STREAM_HEADER = "mifsk/mux_stream.h"
MUX_STREAM_SIGNATURES = {
    "mifsk_mux_stream_create": (_int, [_vp, _int, _u32, _P(_vp)]),
    "mifsk_mux_stream_destroy": (None, [_vp]),
    "mifsk_mux_stream_feed": (_int, [_vp, _P(MuxIO), _vp]),
    "mifsk_mux_stream_seek": (_int, [_vp, _P(_u64), _vp]),
    "mifsk_mux_stream_seen": (_int, [_vp, _P(_u64), _vp]),
    "mifsk_mux_stream_drain": (_u32, [_u32, _u32]),
}

# include/mifsk/squelch.h, the FM stage's power squelch: the fifth extension header, the first that brings
# structs.  Its mirrors, their table and the binding table are names of their own: STRUCTS and the five
# tables above stay as they are.
SQUELCH_HEADER = "mifsk/squelch.h"


class FmSquelchState(C.Structure):
    _fields_ = [("seen", C.c_uint64), ("acc", C.c_uint64), ("span_first", C.c_uint64),
                ("open", C.c_uint32), ("low", C.c_uint32)]


class FmSquelchSpan(C.Structure):
    _fields_ = [("first_window", C.c_uint64), ("end_window", C.c_uint64)]


class FmSquelchIO(C.Structure):
    _fields_ = ROWS_FIELDS + [("kind", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_uint32), ("hang", C.c_uint32),
                              ("open_level", C.c_uint64), ("close_level", C.c_uint64),
                              ("d_state", C.c_void_p), ("d_state_out", C.c_void_p),
                              ("d_energy", C.c_void_p), ("d_gate", C.c_void_p), ("win_stride", C.c_size_t),
                              ("d_nwindows", C.c_void_p), ("d_spans", C.c_void_p), ("d_nspans", C.c_void_p),
                              ("span_cap", C.c_uint32), ("reserved", C.c_uint32),
                              ("d_audio", C.c_void_p), ("audio_stride", C.c_size_t)]


SQUELCH_STRUCTS = {"mifsk_fm_squelch_state": FmSquelchState, "mifsk_fm_squelch_span": FmSquelchSpan,
                   "mifsk_fm_squelch_io": FmSquelchIO}
assert [C.sizeof(t) for t in SQUELCH_STRUCTS.values()] == [32, 16, 152]
assert FmSquelchState.open.offset == 24 and FmSquelchIO.open_level.offset == 48 and FmSquelchIO.d_audio.offset == 136
SQUELCH_SIGNATURES = {
    "mifsk_fm_squelch_batch": (_int, [_vp, _P(FmSquelchIO), _vp]),
    "mifsk_fm_squelch_level": (_u64, [_f64, _u32]),
}

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  minimodem_amd has no fallback path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for table in [SIGNATURES] + list(EXTENSIONS.values()) + [STREAM_SIGNATURES, MUX_STREAM_SIGNATURES, SQUELCH_SIGNATURES]:
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib
