"""ctypes binding of libmodes_gpu.so (include/modes_gpu.h).

Mirrors the reference's interface for this path: a converter (`iq_convert_fn`, convert.h:34-39),
`demodulate2400(struct mag_buf *)` (demod_2400.h:38) and the ifile reader's feed loop
(sdr_ifile.c:169-270).  There is no CPU fallback: if the HIP library or a GPU is missing the
constructor raises.
"""
import ctypes as C
import os

import numpy as np

FMT_UC8, FMT_SC16, FMT_SC16Q11 = 0, 1, 2
_FMT_BYTES = {FMT_UC8: 2, FMT_SC16: 4, FMT_SC16Q11: 4}

# struct mgpu_msg (64 bytes)
MSG_DTYPE = np.dtype([
    ("timestamp", "<i8"), ("sysTimestamp", "<i8"), ("sig_sumsq", "<u8"), ("sig_len", "<u2"),
    ("score", "<i2"), ("phase", "u1"), ("correctedbits", "u1"), ("msgtype", "u1"), ("msgbits", "u1"),
    ("addr", "<u4"), ("msg", "u1", 14), ("raw", "u1", 14),
])
assert MSG_DTYPE.itemsize == 64

# struct mgpu_fields (include/modes_gpu.h): the per-message field decode
FIELDS_DTYPE = np.dtype([
    ("addr", "<u4"), ("AA", "<u4"), ("flags", "<u4"), ("acc_flags", "<u2"), ("nav_flags", "u1"), ("msgtype", "u1"),
    ("addrtype", "u1"), ("source", "u1"), ("airground", "u1"), ("metype", "u1"),
    ("mesub", "u1"), ("CA", "u1"), ("CC", "u1"), ("CF", "u1"),
    ("DR", "u1"), ("FS", "u1"), ("KE", "u1"), ("ND", "u1"),
    ("RI", "u1"), ("SL", "u1"), ("UM", "u1"), ("VS", "u1"),
    ("IID", "u1"), ("category", "u1"), ("emergency", "u1"), ("cpr_type", "u1"),
    ("AC", "<u2"), ("ID", "<u2"), ("squawkHex", "<u2"), ("squawkDec", "<u2"),
    ("baro_alt", "<i4"), ("geom_alt", "<i4"), ("geom_delta", "<i4"), ("baro_rate", "<i4"), ("geom_rate", "<i4"),
    ("ias", "<u2"), ("tas", "<u2"),
    ("heading", "<f4"), ("gs_v0", "<f4"), ("gs_v2", "<f4"), ("gs_selected", "<f4"),
    ("cpr_lat", "<u4"), ("cpr_lon", "<u4"), ("callsign", "S8"),
    ("baro_alt_unit", "u1"), ("geom_alt_unit", "u1"), ("heading_type", "u1"), ("sil_type", "u1"),
    ("nac_p", "u1"), ("nac_v", "u1"), ("sil", "u1"), ("gva", "u1"),
    ("sda", "u1"), ("op_version", "u1"), ("op_hrd", "u1"), ("op_tah", "u1"),
    ("op_flags", "<u2"), ("op_cc_lw", "u1"), ("op_cc_antenna_offset", "u1"),
    ("op_cc_tc", "u1"), ("nav_heading_type", "u1"), ("nav_altitude_source", "u1"), ("nav_modes", "u1"),
    ("nav_fms_altitude", "<u4"), ("nav_mcp_altitude", "<u4"), ("nav_qnh", "<f4"), ("nav_heading", "<f4"),
    ("roll", "<f4"), ("track_rate", "<f4"), ("mach", "<f4"), ("oat", "<f4"), ("humidity", "<f4"), ("wind_direction", "<f4"),
    ("wind_speed", "<u2"), ("static_pressure", "<u2"), ("commb_format", "u1"), ("met_source", "u1"), ("turbulence", "u1"), ("pad0", "u1"),
    ("reserved", "u1", 8),
])
assert FIELDS_DTYPE.itemsize == 176


# struct mgpu_position, mgpu_cpr_case, mgpu_cpr_result (include/modes_gpu.h): CPR pairing and position decode
POSITION_DTYPE = np.dtype([
    ("lat", "<f8"), ("lon", "<f8"), ("partner", "<u4"), ("partner_dt_ms", "<i4"), ("global_result", "i1"), ("local_result", "i1"),
    ("method", "u1"), ("flags", "u1"), ("reserved", "u1", 4),
])
assert POSITION_DTYPE.itemsize == 32
CPR_CASE_DTYPE = np.dtype([
    ("reflat", "<f8"), ("reflon", "<f8"), ("even_lat", "<i4"), ("even_lon", "<i4"), ("odd_lat", "<i4"), ("odd_lon", "<i4"),
    ("fn", "u1"), ("fflag", "u1"), ("surface", "u1"), ("pad", "u1", 5),
])
assert CPR_CASE_DTYPE.itemsize == 40
CPR_RESULT_DTYPE = np.dtype([("lat", "<f8"), ("lon", "<f8"), ("rc", "<i4"), ("pad", "<i4")])
assert CPR_RESULT_DTYPE.itemsize == 24
CPR_NONE, CPR_GLOBAL, CPR_LOCAL_RECEIVER, CPR_LOCAL_AIRCRAFT, CPR_BAD = 0, 1, 2, 3, 4
CPR_NOT_TRIED = 1
CPR_PARTNER_NONE, CPR_PARTNER_EARLIER = 0xFFFFFFFF, 0xFFFFFFFE


class CprConfig(C.Structure):                                         # struct mgpu_cpr_config
    _fields_ = [("ref_lat", C.c_double), ("ref_lon", C.c_double), ("ref_valid", C.c_uint32), ("airborne_max_elapsed_ms", C.c_uint32)]


FILTER_CLOCK_AFTER_FIRST, FILTER_CLOCK_BEFORE_FIRST, FILTER_CLOCK_EXTERNAL = 0, 1, 2


class Config(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("format", C.c_int32), ("nfix_crc", C.c_int32), ("fixDF", C.c_int32),
        ("preamble_threshold", C.c_int32), ("buf_samples", C.c_uint32), ("trailing_samples", C.c_uint32),
        ("mode_ac", C.c_uint32), ("max_samples", C.c_uint64), ("startup_time_ms", C.c_int64),
        ("record_pool_records", C.c_uint64), ("max_messages", C.c_uint64),
        ("filter_clock", C.c_uint32), ("streams_on_device", C.c_uint32), ("chunk_buffers", C.c_uint32), ("abi_version", C.c_uint32),
    ]


class Counters(C.Structure):
    _fields_ = [
        ("demod_preambles", C.c_uint64), ("demod_rejected_bad", C.c_uint64),
        ("demod_rejected_unknown_icao", C.c_uint64), ("demod_accepted", C.c_uint64 * 3),
        ("demod_preamblePhase", C.c_uint64 * 5), ("demod_bestPhase", C.c_uint64 * 5),
        ("strong_signal_count", C.c_uint64), ("signal_power_count", C.c_uint64),
        ("noise_power_count", C.c_uint64), ("samples_processed", C.c_uint64), ("samples_lost", C.c_uint64),
        ("nbuffers", C.c_uint64), ("nflips", C.c_uint64), ("signal_power_sum", C.c_double),
        ("noise_power_sum", C.c_double), ("peak_signal_power", C.c_double), ("demod_modeac", C.c_uint64),
    ]

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out

    @classmethod
    def from_dict(cls, d):
        """The struct of an as_dict() result (the wire form of the counters between ranks is the struct's bytes, as in the C host)."""
        k = cls()
        for name, ctype in cls._fields_:
            v = d[name]
            if hasattr(ctype, "_length_"):
                for i in range(ctype._length_):
                    getattr(k, name)[i] = v[i]
            else:
                setattr(k, name, v)
        return k


class Timing(C.Structure):
    _fields_ = [
        ("h2d_ms", C.c_float), ("convert_ms", C.c_float), ("sweep_ms", C.c_float), ("prescreen_ms", C.c_float),
        ("resolve_ms", C.c_float), ("sigpower_ms", C.c_float), ("d2h_ms", C.c_float), ("total_ms", C.c_float),
        ("n_candidates", C.c_uint64), ("n_records", C.c_uint64), ("n_live_records", C.c_uint64),
        ("n_messages", C.c_uint64), ("n_chunks", C.c_uint64), ("slice_ms", C.c_float), ("build_ms", C.c_float), ("n_timed_chunks", C.c_uint64),
        ("build_wait_ms", C.c_float), ("sweep_fused_chunks", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ShardWalkArgs(C.Structure):
    _fields_ = [
        ("own_first", C.c_uint64), ("flip_after", C.c_void_p), ("nflips", C.c_uint64), ("start_state", C.c_void_p),
        ("start_state_bytes", C.c_uint64), ("check_records", C.c_int32), ("reserved", C.c_int32),
    ]


DEFAULT_CHUNK_BUFFERS = 0                   # mgpu_config.chunk_buffers of Demodulators created without one (tests lower it: more chunks per feed)


class ShardStreamArgs(C.Structure):
    _fields_ = [
        ("first_sample", C.c_uint64), ("history_iq", C.c_void_p), ("own_first", C.c_uint64), ("flip_after", C.c_void_p), ("nflips", C.c_uint64),
        ("start_state", C.c_void_p), ("start_state_bytes", C.c_uint64),
    ]


DEFERRED_DTYPE = np.dtype([("index", "<u8"), ("offset", "<u8")])     # struct mgpu_deferred
BEAST_NET_RULE, BEAST_VERBATIM = 1, 2                                 # MGPU_BEAST_*
BEAST_FRAME_MAX = 44                                                  # bytes of a frame; with receiver ids up to 18 more for the prefix
BEAST_PREFIX_MAX = 18
MERGE_MAX_SEGMENTS = 4096


class BeastArgs(C.Structure):                                         # struct mgpu_beast_args
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("msgs", C.c_void_p), ("n", C.c_uint64), ("verdict", C.c_void_p),
                ("ids", C.c_void_p), ("last_id", C.POINTER(C.c_uint64)), ("out", C.c_void_p), ("cap", C.c_uint64),
                ("bytes", C.POINTER(C.c_uint64)), ("deferred", C.c_void_p), ("deferred_cap", C.c_uint64),
                ("ndeferred", C.POINTER(C.c_uint64))]


SBS_USE_GNSS = 1                                                      # MGPU_SBS_*
RAW_NET_RULE, RAW_VERBATIM, RAW_MLAT = 1, 2, 4                        # MGPU_RAW_*
SBS_LINE_MAX, RAW_LINE_MAX = 176, 43                                  # bytes of a line


class SbsArgs(C.Structure):                                           # struct mgpu_sbs_args
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("msgs", C.c_void_p), ("fields", C.c_void_p), ("positions", C.c_void_p),
                ("verdict", C.c_void_p), ("geom_delta", C.c_void_p), ("n", C.c_uint64), ("now_ms", C.c_int64), ("override_squawk", C.c_int32),
                ("out", C.c_void_p), ("cap", C.c_uint64), ("bytes", C.POINTER(C.c_uint64)), ("deferred", C.c_void_p),
                ("deferred_cap", C.c_uint64), ("ndeferred", C.POINTER(C.c_uint64)), ("nskipped", C.POINTER(C.c_uint64))]


ASTERIX_REMOTE = 1                                                    # MGPU_ASTERIX_*
ASTERIX_RECORD_MAX = 74                                               # bytes of a CAT021 record


class AsterixArgs(C.Structure):                                       # struct mgpu_asterix_args
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("msgs", C.c_void_p), ("fields", C.c_void_p), ("positions", C.c_void_p),
                ("verdict", C.c_void_p), ("ids", C.c_void_p), ("ac_baro_alt", C.c_void_p), ("ac_category", C.c_void_p), ("n", C.c_uint64),
                ("now_ms", C.c_int64), ("out", C.c_void_p), ("cap", C.c_uint64), ("bytes", C.POINTER(C.c_uint64)), ("deferred", C.c_void_p),
                ("deferred_cap", C.c_uint64), ("ndeferred", C.POINTER(C.c_uint64)), ("nskipped", C.POINTER(C.c_uint64))]


class RawArgs(C.Structure):                                           # struct mgpu_raw_args
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("msgs", C.c_void_p), ("verdict", C.c_void_p), ("n", C.c_uint64),
                ("out", C.c_void_p), ("cap", C.c_uint64), ("bytes", C.POINTER(C.c_uint64)), ("deferred", C.c_void_p),
                ("deferred_cap", C.c_uint64), ("ndeferred", C.POINTER(C.c_uint64))]


DUMP_ONLYADDR, DUMP_RAW, DUMP_MLAT, DUMP_QUIET = 1, 2, 4, 8             # MGPU_DUMP_*
DUMP_MAX = 2599                                                       # bytes of a dump (kDumpMax, csrc/dump_format.h)


class DumpArgs(C.Structure):                                          # struct mgpu_dump_args
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("msgs", C.c_void_p), ("fields", C.c_void_p), ("reduce_forward", C.c_void_p),
                ("receiver_ids", C.c_void_p), ("positions", C.c_void_p), ("decoded_nic", C.c_void_p), ("decoded_rc", C.c_void_p), ("n", C.c_uint64),
                ("show_only", C.c_uint32), ("out", C.c_void_p), ("cap", C.c_uint64), ("bytes", C.POINTER(C.c_uint64)), ("deferred", C.c_void_p),
                ("deferred_cap", C.c_uint64), ("ndeferred", C.POINTER(C.c_uint64)), ("nskipped", C.POINTER(C.c_uint64))]


class SnipArgs(C.Structure):                                          # struct mgpu_snip_args
    _fields_ = [("size", C.c_uint32), ("level", C.c_int32), ("iq", C.c_void_p), ("nsamples", C.c_uint64), ("out", C.c_void_p),
                ("cap_samples", C.c_uint64), ("nout", C.POINTER(C.c_uint64)), ("quiet_run", C.POINTER(C.c_uint64)), ("pass_samples", C.c_uint64)]


class UatArgs(C.Structure):                                           # struct mgpu_uat_args
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("text", C.c_void_p), ("nbytes", C.c_uint64), ("out", C.c_void_p), ("cap", C.c_uint64),
                ("msgs", C.c_void_p), ("sig", C.c_void_p), ("line_of", C.c_void_p), ("msgs_cap", C.c_uint64), ("deferred", C.c_void_p), ("deferred_cap", C.c_uint64),
                ("now_ms", C.c_int64), ("bytes", C.POINTER(C.c_uint64)), ("consumed", C.POINTER(C.c_uint64)), ("nlines", C.POINTER(C.c_uint64)),
                ("nframes", C.POINTER(C.c_uint64)), ("nshort", C.POINTER(C.c_uint64)), ("ndeferred", C.POINTER(C.c_uint64)), ("pass_bytes", C.c_uint64)]


UAT_FRAME_TEXT = 45                         # bytes of one AVR line of mgpu_uat_encode


class SbsInArgs(C.Structure):                                         # struct mgpu_sbs_in_args
    _fields_ = [("size", C.c_uint32), ("source", C.c_uint32), ("text", C.c_void_p), ("nbytes", C.c_uint64), ("now_ms", C.c_int64), ("recs", C.c_void_p),
                ("line_of", C.c_void_p), ("recs_cap", C.c_uint64), ("deferred", C.c_void_p), ("deferred_cap", C.c_uint64), ("consumed", C.POINTER(C.c_uint64)),
                ("nlines", C.POINTER(C.c_uint64)), ("nrecs", C.POINTER(C.c_uint64)), ("ninvalid", C.POINTER(C.c_uint64)), ("ndeferred", C.POINTER(C.c_uint64)),
                ("pass_bytes", C.c_uint64)]


SBS_REC_DTYPE = np.dtype([                                            # struct mgpu_sbs_rec: 96 bytes, reserved = 0
    ("sysTimestamp", "<i8"), ("decoded_lat", "<f8"), ("decoded_lon", "<f8"), ("addr", "<u4"), ("flags", "<u4"), ("sbs_flags", "<u4"), ("baro_alt", "<i4"),
    ("baro_rate", "<i4"), ("gs_v0", "<f4"), ("heading", "<f4"), ("squawkDec", "<u4"), ("squawkHex", "<u4"), ("receiverCountMlat", "<i4"), ("mlatEPU", "<i4"),
    ("callsign", "S8"), ("sbsMsgType", "u1"), ("source", "u1"), ("addrtype", "u1"), ("airground", "u1"), ("baro_alt_unit", "u1"), ("heading_type", "u1"),
    ("reserved", "u1", 14)])
assert SBS_REC_DTYPE.itemsize == 96
SBS_SOURCES = {"sbs": 3, "mlat": 4, "jaero": 6, "prio": 11}          # MGPU_SBS_SOURCE_*: the reference's datasource_t
SBS_POS_VALID, SBS_EMERGENCY_VALID, SBS_EMERGENCY = 1, 2, 4           # MGPU_SBS_*


class RawInCounters(C.Structure):                                     # struct mgpu_raw_in_counters
    _fields_ = [("remote_received_modes", C.c_uint64), ("remote_received_modeac", C.c_uint64), ("remote_rejected_unknown_icao", C.c_uint64),
                ("remote_rejected_bad", C.c_uint64), ("remote_accepted", C.c_uint64 * 3)]


class RawInArgs(C.Structure):                                         # struct mgpu_raw_in_args
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("text", C.c_void_p), ("nbytes", C.c_uint64), ("now_ms", C.c_int64), ("msgs", C.c_void_p),
                ("line_of", C.c_void_p), ("signal_level", C.c_void_p), ("msgs_cap", C.c_uint64), ("line_class", C.c_void_p), ("line_class_cap", C.c_uint64),
                ("consumed", C.POINTER(C.c_uint64)), ("nlines", C.POINTER(C.c_uint64)), ("nmsgs", C.POINTER(C.c_uint64)), ("counters", C.POINTER(RawInCounters)),
                ("pass_bytes", C.c_uint64)]


class RawInConfig(C.Structure):                                       # struct mgpu_raw_in_config
    _fields_ = [("size", C.c_uint32), ("nfix_crc", C.c_int32), ("fixDF", C.c_int32), ("mode_ac", C.c_uint32)]


class RawInLine(C.Structure):                                         # struct mgpu_raw_in_line: 88 bytes
    _fields_ = [("msg", C.c_uint8 * 64), ("signal_level", C.c_double), ("cls", C.c_uint32), ("addr", C.c_uint32), ("adder", C.c_uint32), ("reserved", C.c_uint32)]


class BeastInCounters(C.Structure):                                   # struct mgpu_beast_in_counters
    _fields_ = [("remote_received_modes", C.c_uint64), ("remote_received_modeac", C.c_uint64), ("remote_rejected_unknown_icao", C.c_uint64),
                ("remote_rejected_bad", C.c_uint64), ("remote_accepted", C.c_uint64 * 3), ("remote_malformed_beast", C.c_uint64),
                ("nreceiver_ids", C.c_uint64), ("ncommands", C.c_uint64)]


class BeastInConfig(C.Structure):                                     # struct mgpu_beast_in_config
    _fields_ = [("size", C.c_uint32), ("nfix_crc", C.c_int32), ("fixDF", C.c_int32), ("mode_ac", C.c_uint32), ("net_ingest", C.c_uint32), ("reserved", C.c_uint32)]


class BeastInFrame(C.Structure):                                      # struct mgpu_beast_in_frame: 128 bytes
    _fields_ = [("msg", C.c_uint8 * 64), ("signal_level", C.c_double), ("next", C.c_uint64), ("frame_off", C.c_uint64), ("receiver_id", C.c_uint64),
                ("step", C.c_uint32), ("cls", C.c_uint32), ("addr", C.c_uint32), ("adder", C.c_uint32), ("garbage", C.c_uint32), ("id_set", C.c_uint32),
                ("command", C.c_uint32), ("reserved", C.c_uint32)]


class BeastInArgs(C.Structure):                                       # struct mgpu_beast_in_args
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("data", C.c_void_p), ("nbytes", C.c_uint64), ("now_ms", C.c_int64), ("receiver_id_in", C.c_uint64),
                ("net_ingest", C.c_uint32), ("reserved2", C.c_uint32), ("msgs", C.c_void_p), ("receiver_id", C.c_void_p), ("signal_level", C.c_void_p),
                ("frame_of", C.c_void_p), ("msgs_cap", C.c_uint64), ("frame_class", C.c_void_p), ("frame_off", C.c_void_p), ("frames_cap", C.c_uint64),
                ("consumed", C.POINTER(C.c_uint64)), ("nframes", C.POINTER(C.c_uint64)), ("nmsgs", C.POINTER(C.c_uint64)), ("stop", C.POINTER(C.c_uint32)),
                ("stop_off", C.POINTER(C.c_uint64)), ("receiver_id_out", C.POINTER(C.c_uint64)), ("counters", C.POINTER(BeastInCounters)), ("pass_bytes", C.c_uint64)]


def beast_in_counters_dict(cn):
    return dict(remote_received_modes=int(cn.remote_received_modes), remote_received_modeac=int(cn.remote_received_modeac),
                remote_rejected_unknown_icao=int(cn.remote_rejected_unknown_icao), remote_rejected_bad=int(cn.remote_rejected_bad),
                remote_accepted=[int(x) for x in cn.remote_accepted], remote_malformed_beast=int(cn.remote_malformed_beast),
                nreceiver_ids=int(cn.nreceiver_ids), ncommands=int(cn.ncommands))


class PfInCounters(C.Structure):                                      # struct mgpu_pf_in_counters
    _fields_ = [("remote_received_modes", C.c_uint64), ("remote_received_modeac", C.c_uint64), ("remote_rejected_unknown_icao", C.c_uint64),
                ("remote_rejected_bad", C.c_uint64), ("remote_accepted", C.c_uint64 * 3), ("nskipped", C.c_uint64), ("past_end", C.c_uint64)]


class PfInFrame(C.Structure):                                         # struct mgpu_pf_in_frame: 112 bytes
    _fields_ = [("msg", C.c_uint8 * 64), ("signal_level", C.c_double), ("next", C.c_uint64), ("frame_off", C.c_uint64), ("step", C.c_uint32), ("cls", C.c_uint32),
                ("addr", C.c_uint32), ("adder", C.c_uint32), ("past_end", C.c_uint32), ("reserved", C.c_uint32)]


class PfInArgs(C.Structure):                                          # struct mgpu_pf_in_args
    _fields_ = [("size", C.c_uint32), ("look", C.c_uint32), ("data", C.c_void_p), ("nbytes", C.c_uint64), ("now_ms", C.c_int64), ("msgs", C.c_void_p),
                ("signal_level", C.c_void_p), ("frame_of", C.c_void_p), ("msgs_cap", C.c_uint64), ("frame_class", C.c_void_p), ("frame_off", C.c_void_p),
                ("frames_cap", C.c_uint64), ("consumed", C.POINTER(C.c_uint64)), ("nframes", C.POINTER(C.c_uint64)), ("nmsgs", C.POINTER(C.c_uint64)),
                ("counters", C.POINTER(PfInCounters)), ("pass_bytes", C.c_uint64)]


def pf_in_counters_dict(cn):
    return dict(remote_received_modes=int(cn.remote_received_modes), remote_received_modeac=int(cn.remote_received_modeac),
                remote_rejected_unknown_icao=int(cn.remote_rejected_unknown_icao), remote_rejected_bad=int(cn.remote_rejected_bad),
                remote_accepted=[int(x) for x in cn.remote_accepted], nskipped=int(cn.nskipped), past_end=int(cn.past_end))


class RawInFilter(C.Structure):                                       # struct mgpu_raw_in_filter
    _fields_ = [("gen_active", C.c_void_p), ("gen_inactive", C.c_void_p), ("n_active", C.c_uint64), ("n_inactive", C.c_uint64), ("occupied", C.c_uint32),
                ("table_bits", C.c_uint32)]


RAW_NONE, RAW_MODEAC, RAW_BAD, RAW_ACCEPT, RAW_COND, RAW_UNKNOWN = range(6)   # MGPU_RAW_*


class AsterixInArgs(C.Structure):                                     # struct mgpu_asterix_in_args
    _fields_ = [("size", C.c_uint32), ("source", C.c_uint32), ("data", C.c_void_p), ("nbytes", C.c_uint64), ("now_ms", C.c_int64), ("recs", C.c_void_p),
                ("frame_of", C.c_void_p), ("recs_cap", C.c_uint64), ("pass_bytes", C.c_uint64), ("consumed", C.POINTER(C.c_uint64)),
                ("nframes", C.POINTER(C.c_uint64)), ("nrecs", C.POINTER(C.c_uint64)), ("stop", C.POINTER(C.c_uint32)), ("nother", C.POINTER(C.c_uint64)),
                ("nundefined", C.POINTER(C.c_uint64))]


ASTERIX_REC_DTYPE = np.dtype([                                        # struct mgpu_asterix_rec: 128 bytes, reserved = 0
    ("sysTimestamp", "<i8"), ("decoded_lat", "<f8"), ("decoded_lon", "<f8"), ("mach", "<f8"), ("addr", "<u4"), ("flags", "<u4"), ("ast_flags", "<u4"),
    ("baro_alt", "<i4"), ("geom_alt", "<i4"), ("baro_rate", "<i4"), ("geom_rate", "<i4"), ("ias", "<u4"), ("tas", "<u4"), ("squawkHex", "<u4"), ("squawkDec", "<u4"),
    ("category", "<u4"), ("mcp_altitude", "<u4"), ("fms_altitude", "<u4"), ("gs_v0", "<f4"), ("heading", "<f4"), ("roll", "<f4"), ("callsign", "S8"),
    ("source", "u1"), ("addrtype", "u1"), ("airground", "u1"), ("emergency", "u1"), ("nav_modes", "u1"), ("nac_v", "u1"), ("nac_p", "u1"), ("sil", "u1"),
    ("sil_type", "u1"), ("gva", "u1"), ("sda", "u1"), ("nic_baro", "u1"), ("op_version", "u1"), ("heading_type", "u1"), ("baro_alt_unit", "u1"),
    ("geom_alt_unit", "u1"), ("reserved", "u1", 4)])
assert ASTERIX_REC_DTYPE.itemsize == 128
AST_STOP_END, AST_STOP_ZERO_LEN, AST_STOP_CLOSED = 0, 1, 2            # MGPU_AST_STOP_*
AST_POS_VALID = 1                                                     # MGPU_AST_POS_VALID


ABI_VERSION = 6                             # MGPU_ABI_VERSION of the include/modes_gpu.h these ctypes mirrors were written against


class MgpuError(RuntimeError):
    pass


def flip_schedule(end_clocks, startup_ms, filter_clock=0):
    """Indices of the buffers the ICAO filter expires after, from every buffer's end clock (mgpu_flip_schedule: the reference's
    rule, readsb.c:1227-1231)."""
    lib = load_library()
    clocks = np.ascontiguousarray(end_clocks, dtype=np.int64)
    out = np.empty(clocks.size // 1000 + 16, dtype=np.uint64)      # an expiry per 60 s = per ~1099 buffers at least
    n = int(lib.mgpu_flip_schedule(C.c_void_p(clocks.ctypes.data), clocks.size, int(startup_ms), int(filter_clock), C.c_void_p(out.ctypes.data), out.size))
    if n > out.size:
        out = np.empty(n, dtype=np.uint64)
        n = int(lib.mgpu_flip_schedule(C.c_void_p(clocks.ctypes.data), clocks.size, int(startup_ms), int(filter_clock), C.c_void_p(out.ctypes.data), out.size))
    return out[:n].copy()


def expiry_windows(nbuf_total, startup_ms, filter_clock=0, buf_samples=131072):
    """Boolean mask of the buffers an expiry of the ICAO filter can follow (mgpu_expiry_windows)."""
    mask = np.zeros(int(nbuf_total), dtype=np.uint8)
    if nbuf_total:
        load_library().mgpu_expiry_windows(int(nbuf_total), int(buf_samples), int(startup_ms), int(filter_clock), C.c_void_p(mask.ctypes.data))
    return mask.astype(bool)


def shard_round(sched_ts, gathered, nsamples, startup_ms, filter_clock=0, buf_samples=131072):
    """mgpu_shard_round: gathered[r] = (clocks, state_first, state_end) -> (done, next schedule, {rank: rank to import the end state of})."""
    lib = load_library()
    world = len(gathered)
    sched = np.ascontiguousarray(sched_ts, dtype=np.int64)
    clocks = [np.ascontiguousarray(g[0], dtype=np.int64) for g in gathered]
    sf = [np.frombuffer(bytes(g[1]) or b"\0", dtype=np.uint8) for g in gathered]
    se = [np.frombuffer(bytes(g[2]) or b"\0", dtype=np.uint8) for g in gathered]
    ptrs = lambda arrs: (C.c_void_p * world)(*[a.ctypes.data for a in arrs])
    lens = lambda xs: np.array(xs, dtype=np.uint64)
    ncl, nsf, nse = lens([c.size for c in clocks]), lens([len(g[1]) for g in gathered]), lens([len(g[2]) for g in gathered])
    cap = sum(c.size for c in clocks) // 1000 + 64
    nxt = np.empty(cap, dtype=np.int64)
    n_next, done = C.c_uint64(0), C.c_int32(0)
    imp = np.empty(world, dtype=np.int32)
    rc = lib.mgpu_shard_round(sched.ctypes.data if sched.size else None, sched.size, world, ptrs(clocks), C.c_void_p(ncl.ctypes.data), ptrs(sf),
                              C.c_void_p(nsf.ctypes.data), ptrs(se), C.c_void_p(nse.ctypes.data), int(nsamples), int(buf_samples), int(startup_ms),
                              int(filter_clock), C.c_void_p(nxt.ctypes.data), cap, C.byref(n_next), C.c_void_p(imp.ctypes.data), C.byref(done))
    if rc != 0:
        raise MgpuError("mgpu_shard_round failed")
    return bool(done.value), nxt[: n_next.value].copy(), {r: int(imp[r]) for r in range(world) if imp[r] >= 0}


def seqsum(start, terms):
    """((start + t0) + t1) + ... in doubles, in order (mgpu_seqsum)."""
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    return float(load_library().mgpu_seqsum(float(start), C.c_void_p(terms.ctypes.data), terms.size))


SUM_BLOCK_DTYPE = np.dtype([("total", "<u8"), ("e", "<i4"), ("flags", "<u4")])
SUM_BLOCK = 1024                            # messages per block of the block-wise sequential sum


def seqsum_blocks(approx_start, msgs, block=SUM_BLOCK):
    """A range's messages prepared for the block-wise sequential sum of their signal powers (mgpu_seqsum_blocks)."""
    if msgs.dtype != MSG_DTYPE or not msgs.flags["C_CONTIGUOUS"]:
        raise ValueError("seqsum_blocks: need a contiguous mgpu_msg record array")
    out = np.zeros((msgs.size + block - 1) // block, dtype=SUM_BLOCK_DTYPE)
    rc = load_library().mgpu_seqsum_blocks(float(approx_start), C.c_void_p(msgs.ctypes.data), msgs.size, block, C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise MgpuError("mgpu_seqsum_blocks failed")
    return out


def seqsum_blocks_terms(approx_start, sumsq, block=SUM_BLOCK):
    """The same blocks from the messages' 8-byte signal-power numerators (Demodulator.shard_signal_terms)."""
    sumsq = np.ascontiguousarray(sumsq, dtype=np.uint64)
    out = np.zeros((sumsq.size + block - 1) // block, dtype=SUM_BLOCK_DTYPE)
    rc = load_library().mgpu_seqsum_blocks_terms(float(approx_start), C.c_void_p(sumsq.ctypes.data), sumsq.size, block, C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise MgpuError("mgpu_seqsum_blocks_terms failed")
    return out


def seqsum_apply(start, msgs, blocks, block=SUM_BLOCK):
    """-> (the exact sequential sum continued over this range, blocks that had to be re-added message by message)."""
    blocks = np.ascontiguousarray(blocks, dtype=SUM_BLOCK_DTYPE)
    if msgs.dtype != MSG_DTYPE or not msgs.flags["C_CONTIGUOUS"] or blocks.size != (msgs.size + block - 1) // block:
        raise ValueError("seqsum_apply: messages and blocks do not match")
    fb = C.c_uint64(0)
    s = load_library().mgpu_seqsum_apply(float(start), C.c_void_p(msgs.ctypes.data), msgs.size, block, C.c_void_p(blocks.ctypes.data), C.byref(fb))
    return float(s), int(fb.value)


def seqsum_signal_power(start, msgs):
    """... of the messages' signal powers sig_sumsq / 65535^2, in order (mgpu_seqsum_signal_power; demod_2400.c:445-447)."""
    if msgs.dtype != MSG_DTYPE or not msgs.flags["C_CONTIGUOUS"]:
        raise ValueError("seqsum_signal_power: need a contiguous mgpu_msg record array")
    return float(load_library().mgpu_seqsum_signal_power(float(start), C.c_void_p(msgs.ctypes.data), msgs.size))


def lib_path():
    """The product library; MGPU_LIBRARY=libmodes_gpu_exp.so selects the cross-check build (`make -C readsb_amd/csrc exp`:
    the same library plus the superseded fused sweep kernel) — tests and tools only."""
    name = os.path.basename(os.environ.get("MGPU_LIBRARY", "libmodes_gpu.so"))
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", name)


_lib = None


def load_library():
    """dlopen libmodes_gpu.so (built in-tree by __graft_entry__.build()).  Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise MgpuError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    vp, u64, u32, i32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int64
    lib.mgpu_config_defaults_abi.argtypes = [C.POINTER(Config), u32, u32]
    lib.mgpu_config_defaults_abi.restype = None
    lib.mgpu_abi_version.restype = u32
    # this file mirrors the structs of include/modes_gpu.h at ABI_VERSION: a library of another version is refused here, and
    # mgpu_create checks the version the defaults call wrote into the struct (never more than sizeof(Config) bytes of it)
    if lib.mgpu_abi_version() != ABI_VERSION:
        raise MgpuError(f"{path} is ABI version {lib.mgpu_abi_version()}, readsb_amd/binding.py mirrors version {ABI_VERSION}: rebuild the library")
    lib.mgpu_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.mgpu_destroy.argtypes = [vp]
    lib.mgpu_destroy.restype = None
    lib.mgpu_reset.argtypes = [vp]
    lib.mgpu_strerror.argtypes = [i32]
    lib.mgpu_strerror.restype = C.c_char_p
    lib.mgpu_last_error.argtypes = [vp]
    lib.mgpu_last_error.restype = C.c_char_p
    lib.mgpu_device_count.restype = i32
    lib.mgpu_set_deferred.argtypes = [vp, i32]
    lib.mgpu_set_device_messages.argtypes = [vp, i32]
    lib.mgpu_collect_device.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), vp]
    lib.mgpu_feed_iq.argtypes = [vp, vp, u64]
    lib.mgpu_feed_iq_device.argtypes = [vp, vp, u64]
    lib.mgpu_host_cpus.argtypes = [vp, vp, i32]
    lib.mgpu_host_alloc.argtypes = [vp, u64]
    lib.mgpu_host_alloc.restype = vp
    lib.mgpu_host_free.argtypes = [vp, vp]
    lib.mgpu_host_free.restype = None
    lib.mgpu_host_register.argtypes = [vp, vp, u64]
    lib.mgpu_host_unregister.argtypes = [vp, vp]
    lib.mgpu_upload_iq.argtypes = [vp, vp, u64]
    lib.mgpu_device_iq_buffer.argtypes = [vp]
    lib.mgpu_device_iq_buffer.restype = vp
    lib.mgpu_finish.argtypes = [vp]
    lib.mgpu_collect.argtypes = [vp, vp, u64, C.POINTER(u64), C.POINTER(Counters)]
    lib.mgpu_pending_messages.argtypes = [vp]
    lib.mgpu_filter_expire.argtypes = [vp]
    lib.mgpu_filter_add.argtypes = [vp, u32]
    lib.mgpu_set_message_buffer.argtypes = [vp, vp, u64]
    lib.mgpu_set_device_message_buffer.argtypes = [vp, vp, u64]
    lib.mgpu_decode_fields.argtypes = [vp, vp, u64, vp]
    lib.mgpu_decode_fields_device.argtypes = [vp, vp, u64, vp]
    lib.mgpu_track_gate.argtypes = [vp, vp, u64, vp]
    lib.mgpu_track_gate_device.argtypes = [vp, vp, vp, u64, vp]
    lib.mgpu_track_gate_reset.argtypes = [vp]
    lib.mgpu_cpr_track.argtypes = [vp, C.POINTER(CprConfig), vp, u64, vp]
    lib.mgpu_cpr_track_device.argtypes = [vp, C.POINTER(CprConfig), vp, vp, u64, vp]
    lib.mgpu_cpr_reset.argtypes = [vp]
    lib.mgpu_cpr_decode.argtypes = [vp, vp, u64, vp]
    lib.mgpu_cpr_decode_device.argtypes = [vp, vp, u64, vp]
    lib.mgpu_beast_encode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    lib.mgpu_beast_encode_gated.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]
    lib.mgpu_beast_encode_gated_device.argtypes = [vp, vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]
    lib.mgpu_beast_encode_device.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    lib.mgpu_beast_encode_ex.argtypes = [vp, C.POINTER(BeastArgs)]
    lib.mgpu_beast_encode_ex_device.argtypes = [vp, C.POINTER(BeastArgs)]
    lib.mgpu_sbs_encode_ex.argtypes = [vp, C.POINTER(SbsArgs)]
    lib.mgpu_sbs_encode_ex_device.argtypes = [vp, C.POINTER(SbsArgs)]
    lib.mgpu_asterix_encode_ex.argtypes = [vp, C.POINTER(AsterixArgs)]
    lib.mgpu_asterix_encode_ex_device.argtypes = [vp, C.POINTER(AsterixArgs)]
    lib.mgpu_raw_encode_ex.argtypes = [vp, C.POINTER(RawArgs)]
    lib.mgpu_raw_encode_ex_device.argtypes = [vp, C.POINTER(RawArgs)]
    lib.mgpu_dump_encode_ex.argtypes = [vp, C.POINTER(DumpArgs)]
    lib.mgpu_dump_encode_ex_device.argtypes = [vp, C.POINTER(DumpArgs)]
    lib.mgpu_dump_format_host.argtypes = [C.POINTER(DumpArgs), u64, vp, u64]
    lib.mgpu_dump_format_host.restype = C.c_int64
    lib.mgpu_uat_encode.argtypes = [vp, C.POINTER(UatArgs)]
    lib.mgpu_uat_encode_device.argtypes = [vp, C.POINTER(UatArgs)]
    lib.mgpu_uat_format_host.argtypes = [C.POINTER(UatArgs), u64, vp, u64, vp, vp]
    lib.mgpu_uat_format_host.restype = C.c_int64
    lib.mgpu_uat_format_line_host.argtypes = [vp, u64, C.c_int64, vp, u64, vp, vp]
    lib.mgpu_uat_format_line_host.restype = C.c_int64
    lib.mgpu_sbs_decode.argtypes = [vp, C.POINTER(SbsInArgs)]
    lib.mgpu_sbs_decode_device.argtypes = [vp, C.POINTER(SbsInArgs)]
    lib.mgpu_sbs_parse_host.argtypes = [C.POINTER(SbsInArgs), u64, vp]
    lib.mgpu_raw_decode.argtypes = [vp, C.POINTER(RawInArgs)]
    lib.mgpu_raw_decode_device.argtypes = [vp, C.POINTER(RawInArgs)]
    lib.mgpu_raw_parse_line_host.argtypes = [vp, u64, C.c_int64, C.POINTER(RawInConfig), C.POINTER(RawInLine)]
    lib.mgpu_raw_decode_host.argtypes = [C.POINTER(RawInArgs), C.POINTER(RawInConfig), C.POINTER(RawInFilter)]
    lib.mgpu_beast_decode.argtypes = [vp, C.POINTER(BeastInArgs)]
    lib.mgpu_beast_decode_device.argtypes = [vp, C.POINTER(BeastInArgs)]
    lib.mgpu_beast_parse_host.argtypes = [vp, u64, u64, C.c_int64, C.POINTER(BeastInConfig), C.POINTER(BeastInFrame)]
    lib.mgpu_beast_decode_host.argtypes = [C.POINTER(BeastInArgs), C.POINTER(RawInConfig), C.POINTER(RawInFilter)]
    lib.mgpu_pf_decode.argtypes = [vp, C.POINTER(PfInArgs)]
    lib.mgpu_pf_decode_device.argtypes = [vp, C.POINTER(PfInArgs)]
    lib.mgpu_pf_parse_host.argtypes = [vp, u64, u64, C.c_int64, C.POINTER(RawInConfig), C.POINTER(PfInFrame)]
    lib.mgpu_pf_decode_host.argtypes = [C.POINTER(PfInArgs), C.POINTER(RawInConfig), C.POINTER(RawInFilter)]
    lib.mgpu_asterix_decode.argtypes = [vp, C.POINTER(AsterixInArgs)]
    lib.mgpu_asterix_decode_device.argtypes = [vp, C.POINTER(AsterixInArgs)]
    lib.mgpu_asterix_parse_host.argtypes = [C.POINTER(AsterixInArgs), u64, vp]
    lib.mgpu_asterix_parse_record_host.argtypes = [vp, u64, u64, C.c_uint32, C.c_int64, vp]
    lib.mgpu_sbs_parse_line_host.argtypes = [vp, u64, C.c_uint32, C.c_int64, vp]
    lib.mgpu_snip.argtypes = [vp, C.POINTER(SnipArgs)]
    lib.mgpu_snip_device.argtypes = [vp, C.POINTER(SnipArgs)]
    lib.mgpu_merge_by_time.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    lib.mgpu_merge_by_time_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    lib.mgpu_merge_last_passes.argtypes = [vp]
    lib.mgpu_shard_begin.argtypes = [vp, u64, vp, i32]
    lib.mgpu_adder_bitmap_get.argtypes = [vp, vp]
    lib.mgpu_adder_bitmap_set.argtypes = [vp, vp]
    lib.mgpu_shard_packets.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    lib.mgpu_walk_packets.argtypes = [vp, vp, u64]
    lib.mgpu_shard_clock_estimate.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
    lib.mgpu_shard_walk.argtypes = [vp, vp, u64, C.POINTER(ShardWalkArgs), vp, u64, C.POINTER(u64)]
    lib.mgpu_shard_state.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u64)]
    lib.mgpu_shard_stream_begin.argtypes = [vp, C.POINTER(ShardStreamArgs)]
    lib.mgpu_shard_stream_mark.argtypes = [vp]
    lib.mgpu_shard_stream_end.argtypes = [vp, vp, u64, C.POINTER(u64)]
    lib.mgpu_shard_noise_terms.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    lib.mgpu_shard_signal_terms.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    lib.mgpu_seqsum_blocks_terms.argtypes = [C.c_double, vp, u64, u32, vp]
    lib.mgpu_flip_schedule.argtypes = [vp, u64, i64, i32, vp, u64]
    lib.mgpu_flip_schedule.restype = u64
    lib.mgpu_expiry_windows.argtypes = [u64, u32, i64, i32, vp]
    lib.mgpu_expiry_windows.restype = u64
    lib.mgpu_shard_round.argtypes = [vp, u64, u32, vp, vp, vp, vp, vp, vp, u64, u32, i64, i32, vp, u64, C.POINTER(u64), vp, C.POINTER(i32)]
    lib.mgpu_seqsum.argtypes = [C.c_double, vp, u64]
    lib.mgpu_seqsum.restype = C.c_double
    lib.mgpu_seqsum_signal_power.argtypes = [C.c_double, vp, u64]
    lib.mgpu_seqsum_signal_power.restype = C.c_double
    lib.mgpu_seqsum_blocks.argtypes = [C.c_double, vp, u64, u32, vp]
    lib.mgpu_seqsum_apply.argtypes = [C.c_double, vp, u64, u32, vp, C.POINTER(u64)]
    lib.mgpu_seqsum_apply.restype = C.c_double
    lib.mgpu_pending_messages.restype = u64
    lib.mgpu_last_timing.argtypes = [vp, C.POINTER(Timing)]
    lib.mgpu_debug_device_walk.argtypes = [vp, C.POINTER(u64)]
    lib.mgpu_debug_last_magnitudes.argtypes = [vp, vp, u64]
    lib.mgpu_event_bracket_us.argtypes = [vp, C.POINTER(C.c_float)]
    lib.mgpu_convert.argtypes = [vp, vp, vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mgpu_demod_mag_buf.argtypes = [vp, vp, u32, i64, i64, C.c_double, u32]
    lib.mgpu_demod_mag_buf_ac.argtypes = [vp, vp, u32, i64, i64, C.c_double, C.c_double, u32]
    lib.mgpu_crc_checksum.argtypes = [vp, i32]
    lib.mgpu_crc_checksum.restype = u32
    lib.mgpu_crc_diagnose.argtypes = [i32, u32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.mgpu_crc_table_size.argtypes = [i32, i32]
    lib.mgpu_uc8_table.restype = C.POINTER(C.c_uint16)
    _lib = lib
    return lib


class Demodulator:
    """One SDR stream on one GPU (struct mgpu_ctx)."""
    shard_counters_complete = True      # mgpu_walk_packets rebuilds every statistic of an unsharded run (shard packets carry what it needs)

    def __init__(self, fmt=FMT_UC8, nfix_crc=1, fix_df=1, preamble_threshold=58, max_samples=64 * 131072,
                 device=0, startup_time_ms=0, record_pool_records=0, max_messages=0, buf_samples=131072, mode_ac=0,
                 filter_clock=0, chunk_buffers=None):
        self.lib = load_library()
        cfg = Config()
        self.lib.mgpu_config_defaults_abi(C.byref(cfg), C.sizeof(Config), ABI_VERSION)
        cfg.device, cfg.format, cfg.nfix_crc, cfg.fixDF = device, fmt, nfix_crc, fix_df
        cfg.preamble_threshold, cfg.max_samples, cfg.startup_time_ms = preamble_threshold, max_samples, startup_time_ms
        cfg.record_pool_records, cfg.max_messages, cfg.buf_samples = record_pool_records, max_messages, buf_samples
        cfg.mode_ac = 1 if mode_ac else 0
        cfg.filter_clock = filter_clock          # FILTER_CLOCK_*: who runs icaoFilterExpire (modes_gpu.h)
        cfg.chunk_buffers = DEFAULT_CHUNK_BUFFERS if chunk_buffers is None else chunk_buffers   # buffers per pipeline chunk (0 = the library's 1024)
        self.cfg = cfg
        self.fmt = fmt
        self._collect_buf = None
        self._msgbuf = None
        self.ctx = C.c_void_p()
        rc = self.lib.mgpu_create(C.byref(cfg), C.byref(self.ctx))
        if rc != 0:
            raise MgpuError(f"mgpu_create: {self.lib.mgpu_strerror(rc).decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.mgpu_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise MgpuError(f"{what}: {self.lib.mgpu_strerror(rc).decode()} ({self.lib.mgpu_last_error(self.ctx).decode()})")

    def _nsamples(self, iq):
        iq = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
        return iq, iq.size // _FMT_BYTES[self.fmt]

    def reset(self):
        self._chk(self.lib.mgpu_reset(self.ctx), "mgpu_reset")

    def filter_expire(self):
        """icaoFilterExpire() forwarded by the host (filter_clock=FILTER_CLOCK_EXTERNAL only)."""
        self._chk(self.lib.mgpu_filter_expire(self.ctx), "mgpu_filter_expire")

    def filter_add(self, addr):
        """icaoFilterAdd(addr) made by the host outside the demodulator."""
        self._chk(self.lib.mgpu_filter_add(self.ctx, int(addr)), "mgpu_filter_add")

    def feed_iq(self, iq):
        iq, n = self._nsamples(iq)
        self._chk(self.lib.mgpu_feed_iq(self.ctx, iq.ctypes.data, n), "mgpu_feed_iq")

    def upload_iq(self, iq):
        iq, n = self._nsamples(iq)
        self._chk(self.lib.mgpu_upload_iq(self.ctx, iq.ctypes.data, n), "mgpu_upload_iq")
        return n

    def device_iq_buffer(self):
        return self.lib.mgpu_device_iq_buffer(self.ctx)

    def feed_resident(self, nsamples, dptr=None):
        self._chk(self.lib.mgpu_feed_iq_device(self.ctx, dptr if dptr is not None else self.device_iq_buffer(), nsamples),
                  "mgpu_feed_iq_device")

    def finish(self):
        self._chk(self.lib.mgpu_finish(self.ctx), "mgpu_finish")

    def set_message_buffer(self, arr):
        """Build the messages of the following feeds straight into `arr` (a contiguous mgpu_msg record array);
        collect(out=arr) then only reports how many there are.  None returns to the internal list."""
        if arr is None:
            self._chk(self.lib.mgpu_set_message_buffer(self.ctx, None, 0), "mgpu_set_message_buffer")
            self._msgbuf = None
            return
        if arr.dtype != MSG_DTYPE or not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("set_message_buffer: need a contiguous mgpu_msg record array")
        self._chk(self.lib.mgpu_set_message_buffer(self.ctx, C.c_void_p(arr.ctypes.data), C.c_uint64(arr.size)), "mgpu_set_message_buffer")
        self._msgbuf = arr                   # keep it alive

    # ---- one capture sharded by buffer ranges (include/modes_gpu.h, "sharded" section; readsb_amd/shard.py) ----
    def shard_begin(self, first_sample, history_iq, mode):
        hist = None if history_iq is None else np.ascontiguousarray(history_iq, dtype=np.uint8)
        self._hist_keep = hist
        self._chk(self.lib.mgpu_shard_begin(self.ctx, C.c_uint64(first_sample), None if hist is None else C.c_void_p(hist.ctypes.data), mode),
                  "mgpu_shard_begin")

    def adder_bitmap(self):
        words = np.empty(1 << 19, dtype=np.uint32)
        self._chk(self.lib.mgpu_adder_bitmap_get(self.ctx, C.c_void_p(words.ctypes.data)), "mgpu_adder_bitmap_get")
        return words

    def set_adder_bitmap(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert words.size == 1 << 19
        self._chk(self.lib.mgpu_adder_bitmap_set(self.ctx, C.c_void_p(words.ctypes.data)), "mgpu_adder_bitmap_set")

    def shard_packets(self):
        p, n = C.c_void_p(), C.c_uint64(0)
        self._chk(self.lib.mgpu_shard_packets(self.ctx, C.byref(p), C.byref(n)), "mgpu_shard_packets")
        if not n.value:
            return np.zeros(0, dtype=np.uint8)
        # (a view of the library's own buffer: valid until the context's next shard pass or reset)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,))

    def walk_packets(self, packets):
        packets = np.ascontiguousarray(packets, dtype=np.uint8)
        self._chk(self.lib.mgpu_walk_packets(self.ctx, C.c_void_p(packets.ctypes.data), C.c_uint64(packets.size)), "mgpu_walk_packets")

    # ---- ... with the ordered walk itself sharded over the ranks (include/modes_gpu.h, "round 4"; shard.py: ShardWalkRank) ----
    @staticmethod
    def _packets_arg(packets):
        if packets is None:
            return None, 0, None
        packets = np.ascontiguousarray(packets, dtype=np.uint8)
        return C.c_void_p(packets.ctypes.data), packets.size, packets

    def shard_clock_estimate(self, own_first, nbuffers, packets=None):
        """The range's buffers' end clocks estimated from the records alone (packets=None: the context's own packets)."""
        ptr, size, keep = self._packets_arg(packets)
        out = np.empty(int(nbuffers) + 1, dtype=np.int64)
        n = C.c_uint64(0)
        self._chk(self.lib.mgpu_shard_clock_estimate(self.ctx, ptr, size, int(own_first), C.c_void_p(out.ctypes.data), out.size, C.byref(n)),
                  "mgpu_shard_clock_estimate")
        return out[: n.value]

    def shard_walk(self, own_first, nbuffers, flip_after_ts, start_state=None, packets=None, check_records=False):
        """Walk warm-up + range with the expiry schedule imposed, build the range's messages (mgpu_shard_walk).
        -> (end clocks of the range's buffers, state at own_first, state at the range's end) — the states as bytes."""
        ptr, size, keep = self._packets_arg(packets)
        sched = np.ascontiguousarray(flip_after_ts, dtype=np.int64)
        a = ShardWalkArgs()
        a.own_first = int(own_first)
        a.flip_after = sched.ctypes.data if sched.size else None
        a.nflips = sched.size
        st = None
        if start_state is not None:
            st = np.frombuffer(start_state, dtype=np.uint8)
            a.start_state, a.start_state_bytes = st.ctypes.data, st.size
        a.check_records = 1 if check_records else 0
        out = np.empty(int(nbuffers) + 1, dtype=np.int64)
        n = C.c_uint64(0)
        self._chk(self.lib.mgpu_shard_walk(self.ctx, ptr, size, C.byref(a), C.c_void_p(out.ctypes.data), out.size, C.byref(n)), "mgpu_shard_walk")
        states = []
        for which in (0, 1):
            bp, bn = C.c_void_p(), C.c_uint64(0)
            self._chk(self.lib.mgpu_shard_state(self.ctx, which, C.byref(bp), C.byref(bn)), "mgpu_shard_state")
            states.append(C.string_at(bp, bn.value) if bn.value else b"")
        return out[: n.value].copy(), states[0], states[1]

    def _shard_states(self):
        states = []
        for which in (0, 1):
            bp, bn = C.c_void_p(), C.c_uint64(0)
            self._chk(self.lib.mgpu_shard_state(self.ctx, which, C.byref(bp), C.byref(bn)), "mgpu_shard_state")
            states.append(C.string_at(bp, bn.value) if bn.value else b"")
        return states

    def shard_stream_begin(self, first_sample, history_iq, own_first, flip_after_ts, start_state=None):
        """A rank's pass through the ordinary pipeline (mgpu_shard_stream_*): resets the context, cold start or imported state."""
        hist = None if history_iq is None else np.ascontiguousarray(history_iq, dtype=np.uint8)
        sched = np.ascontiguousarray(flip_after_ts, dtype=np.int64)
        a = ShardStreamArgs()
        a.first_sample, a.own_first = int(first_sample), int(own_first)
        a.history_iq = None if hist is None else hist.ctypes.data
        a.flip_after, a.nflips = (sched.ctypes.data if sched.size else None), sched.size
        st = None
        if start_state is not None:
            st = np.frombuffer(start_state, dtype=np.uint8)
            a.start_state, a.start_state_bytes = st.ctypes.data, st.size
        self._chk(self.lib.mgpu_shard_stream_begin(self.ctx, C.byref(a)), "mgpu_shard_stream_begin")

    def shard_stream_mark(self):
        self._chk(self.lib.mgpu_shard_stream_mark(self.ctx), "mgpu_shard_stream_mark")

    def shard_stream_end(self, nbuffers):
        """-> (the range's true end clocks, state at own_first, state at the range's end)."""
        out = np.empty(int(nbuffers) + 1, dtype=np.int64)
        n = C.c_uint64(0)
        self._chk(self.lib.mgpu_shard_stream_end(self.ctx, C.c_void_p(out.ctypes.data), out.size, C.byref(n)), "mgpu_shard_stream_end")
        s0, s1 = self._shard_states()
        return out[: n.value].copy(), s0, s1

    def shard_noise_terms(self):
        """What each buffer of the walked range adds to noise_power_sum, in order (a copy)."""
        tp, tn = C.c_void_p(), C.c_uint64(0)
        self._chk(self.lib.mgpu_shard_noise_terms(self.ctx, C.byref(tp), C.byref(tn)), "mgpu_shard_noise_terms")
        if not tn.value:
            return np.zeros(0, dtype=np.float64)
        return np.ctypeslib.as_array(C.cast(tp, C.POINTER(C.c_double)), shape=(tn.value,)).copy()

    def shard_signal_terms(self):
        """sig_sumsq of every accepted message of the walked range, in order (a view of the library's own array: valid until the
        context's next shard pass); empty with Mode A/C."""
        tp, tn = C.c_void_p(), C.c_uint64(0)
        self._chk(self.lib.mgpu_shard_signal_terms(self.ctx, C.byref(tp), C.byref(tn)), "mgpu_shard_signal_terms")
        if not tn.value:
            return np.zeros(0, dtype=np.uint64)
        return np.ctypeslib.as_array(C.cast(tp, C.POINTER(C.c_uint64)), shape=(tn.value,))

    def decode_fields(self, msgs):
        """Per-message field records (FIELDS_DTYPE) of a message record array, decoded on the GPU."""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        out = np.empty(len(msgs), dtype=FIELDS_DTYPE)
        self._chk(self.lib.mgpu_decode_fields(self.ctx, C.c_void_p(msgs.ctypes.data), len(msgs), C.c_void_p(out.ctypes.data)), "mgpu_decode_fields")
        return out

    def decode_fields_device(self, d_msgs_ptr, n, d_out_ptr):
        self._chk(self.lib.mgpu_decode_fields_device(self.ctx, C.c_void_p(d_msgs_ptr), n, C.c_void_p(d_out_ptr)), "mgpu_decode_fields_device")

    def track_gate(self, msgs):
        """First stage of the tracker + the forwarding rule on the GPU (include/modes_gpu.h): one verdict byte per message — bits 0-1
        0 not forwarded / 1 forwarded / 2 deferred to the host's tracker.  msgs: accepted messages in order, whole sample buffers
        per call; the aircraft table lives on the device from call to call (track_gate_reset)."""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        out = np.empty(len(msgs), dtype=np.uint8)
        self._chk(self.lib.mgpu_track_gate(self.ctx, C.c_void_p(msgs.ctypes.data), len(msgs), C.c_void_p(out.ctypes.data)), "mgpu_track_gate")
        return out

    def beast_encode_gated(self, msgs, net_rule=False, deferred_cap=None, verbatim=False, receiver_ids=None, last_id=0):
        """mgpu_beast_encode_gated: -> (the beast stream of the certainly-forwarded messages, deferred[] records {index, offset}).
        verbatim / receiver_ids / last_id: the gate's verdicts (track_gate, continuing the aircraft table just the same) through
        beast_encode_ex; with receiver_ids the result has the writer's id behind the list as a third member."""
        if verbatim or receiver_ids is not None:
            verdict = self.track_gate(msgs)
            stream, deferred, last = self.beast_encode_ex(msgs, verdict=verdict, net_rule=net_rule, verbatim=verbatim, ids=receiver_ids, last_id=last_id,
                                                          deferred_cap=deferred_cap)
            return (stream, deferred) if receiver_ids is None else (stream, deferred, last)
        msgs = np.ascontiguousarray(msgs)
        n = len(msgs)
        cap = n * 44 + 64
        dcap = int(deferred_cap if deferred_cap is not None else n)
        out = np.empty(cap, dtype=np.uint8)
        deferred = np.zeros(max(dcap, 1), dtype=DEFERRED_DTYPE)
        nb, nd = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.mgpu_beast_encode_gated(self.ctx, C.c_void_p(msgs.ctypes.data), C.c_uint64(n), C.c_uint32(1 if net_rule else 0),
                                                   C.c_void_p(out.ctypes.data), C.c_uint64(cap), C.byref(nb), C.c_void_p(deferred.ctypes.data),
                                                   C.c_uint64(dcap), C.byref(nd)), "mgpu_beast_encode_gated")
        return out[: nb.value].tobytes(), deferred[: nd.value].copy()

    def track_gate_device(self, d_msgs_ptr, d_fields_ptr, n, d_verdict_ptr):
        self._chk(self.lib.mgpu_track_gate_device(self.ctx, C.c_void_p(d_msgs_ptr), C.c_void_p(d_fields_ptr), n, C.c_void_p(d_verdict_ptr)), "mgpu_track_gate_device")

    def track_gate_reset(self):
        self._chk(self.lib.mgpu_track_gate_reset(self.ctx), "mgpu_track_gate_reset")

    @staticmethod
    def _cpr_config(ref, airborne_max_elapsed_ms):
        cfg = CprConfig(0.0, 0.0, 0, int(airborne_max_elapsed_ms))
        if ref is not None:
            cfg.ref_lat, cfg.ref_lon, cfg.ref_valid = float(ref[0]), float(ref[1]), 1
        return cfg

    def cpr_track(self, msgs, ref=None, airborne_max_elapsed_ms=0):
        """CPR pairing and position decode on the GPU (include/modes_gpu.h, mgpu_cpr_track): one POSITION_DTYPE record per message.
        ref: the receiver's (lat, lon) or None; the aircraft table lives on the device from call to call (cpr_reset)."""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        out = np.empty(len(msgs), dtype=POSITION_DTYPE)
        cfg = self._cpr_config(ref, airborne_max_elapsed_ms)
        self._chk(self.lib.mgpu_cpr_track(self.ctx, C.byref(cfg), C.c_void_p(msgs.ctypes.data), len(msgs), C.c_void_p(out.ctypes.data)), "mgpu_cpr_track")
        return out

    def cpr_track_device(self, d_msgs_ptr, d_fields_ptr, n, d_out_ptr, ref=None, airborne_max_elapsed_ms=0):
        cfg = self._cpr_config(ref, airborne_max_elapsed_ms)
        self._chk(self.lib.mgpu_cpr_track_device(self.ctx, C.byref(cfg), C.c_void_p(d_msgs_ptr), C.c_void_p(d_fields_ptr), n, C.c_void_p(d_out_ptr)),
                  "mgpu_cpr_track_device")

    def cpr_reset(self):
        self._chk(self.lib.mgpu_cpr_reset(self.ctx), "mgpu_cpr_reset")

    def cpr_decode(self, cases):
        """cpr.c's decoders on the GPU, one CPR_CASE_DTYPE record per case -> CPR_RESULT_DTYPE records."""
        cases = np.ascontiguousarray(cases)
        assert cases.dtype == CPR_CASE_DTYPE
        out = np.empty(len(cases), dtype=CPR_RESULT_DTYPE)
        self._chk(self.lib.mgpu_cpr_decode(self.ctx, C.c_void_p(cases.ctypes.data), len(cases), C.c_void_p(out.ctypes.data)), "mgpu_cpr_decode")
        return out

    def cpr_decode_device(self, d_cases_ptr, n, d_out_ptr):
        self._chk(self.lib.mgpu_cpr_decode_device(self.ctx, C.c_void_p(d_cases_ptr), n, C.c_void_p(d_out_ptr)), "mgpu_cpr_decode_device")

    def beast_encode(self, msgs, verbatim=False, receiver_ids=None, last_id=0):
        """Beast wire stream (bytes) of a record array (host memory in, host memory out, encoded on the GPU).  verbatim /
        receiver_ids / last_id: beast_encode_ex's; with receiver_ids the result is (bytes, the writer's id behind the list)."""
        if verbatim or receiver_ids is not None:
            stream, _, last = self.beast_encode_ex(msgs, verbatim=verbatim, ids=receiver_ids, last_id=last_id)
            return stream if receiver_ids is None else (stream, last)
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        out = np.empty(len(msgs) * 44 + 64, dtype=np.uint8)
        nb = C.c_uint64(0)
        self._chk(self.lib.mgpu_beast_encode(self.ctx, C.c_void_p(msgs.ctypes.data), len(msgs), C.c_void_p(out.ctypes.data), out.size, C.byref(nb)),
                  "mgpu_beast_encode")
        return out[: nb.value].tobytes()

    @staticmethod
    def _beast_flags(net_rule, verbatim):
        return (BEAST_NET_RULE if net_rule else 0) | (BEAST_VERBATIM if verbatim else 0)

    def beast_encode_ex(self, msgs, verdict=None, net_rule=False, verbatim=False, ids=None, last_id=0, deferred_cap=None):
        """mgpu_beast_encode_ex on host arrays: the encoder with --net-verbatim (payload from raw[], every carried message framed) and
        --net-receiver-id (ids: one u64 per message; last_id: the writer's id before the list, 0 for a fresh one).  verdict: the
        caller's gate bytes or None (every message).  -> (stream bytes, deferred[] records, the writer's id behind the list)."""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        n = len(msgs)
        cap = n * (BEAST_FRAME_MAX + (BEAST_PREFIX_MAX if ids is not None else 0)) + 64
        out = np.empty(cap, dtype=np.uint8)
        dcap = int(deferred_cap if deferred_cap is not None else (n if verdict is not None else 0))
        deferred = np.zeros(max(dcap, 1), dtype=DEFERRED_DTYPE)
        if verdict is not None:
            verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
            assert len(verdict) == n
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            assert len(ids) == n
        nb, nd, last = C.c_uint64(0), C.c_uint64(0), C.c_uint64(int(last_id))
        a = BeastArgs(C.sizeof(BeastArgs), self._beast_flags(net_rule, verbatim), msgs.ctypes.data, n,
                      verdict.ctypes.data if verdict is not None else None, ids.ctypes.data if ids is not None else None, C.pointer(last),
                      out.ctypes.data, cap, C.pointer(nb), deferred.ctypes.data, dcap, C.pointer(nd))
        self._chk(self.lib.mgpu_beast_encode_ex(self.ctx, C.byref(a)), "mgpu_beast_encode_ex")
        return out[: nb.value].tobytes(), deferred[: nd.value].copy(), int(last.value)

    def beast_encode_ex_device(self, d_msgs_ptr, n, d_out_ptr, cap, d_verdict_ptr=None, net_rule=False, verbatim=False, d_ids_ptr=None, last_id=0,
                               d_deferred_ptr=None, deferred_cap=0):
        """mgpu_beast_encode_ex_device: everything in HBM (pointers as ints).  -> (the stream's size in bytes, the number of
        deferred messages, the writer's id behind the list)."""
        nb, nd, last = C.c_uint64(0), C.c_uint64(0), C.c_uint64(int(last_id))
        a = BeastArgs(C.sizeof(BeastArgs), self._beast_flags(net_rule, verbatim), d_msgs_ptr, n, d_verdict_ptr, d_ids_ptr, C.pointer(last), d_out_ptr, cap,
                      C.pointer(nb), d_deferred_ptr, deferred_cap, C.pointer(nd))
        self._chk(self.lib.mgpu_beast_encode_ex_device(self.ctx, C.byref(a)), "mgpu_beast_encode_ex_device")
        return int(nb.value), int(nd.value), int(last.value)

    def sbs_encode(self, msgs, now_ms, fields=None, positions=None, verdict=None, geom_delta=None, use_gnss=False, override_squawk=-1, deferred_cap=None):
        """mgpu_sbs_encode_ex on host arrays: the BaseStation lines of a record array (include/modes_gpu.h).  fields: decode_fields'
        records or None (decoded by the library); positions: cpr_track's records or None; verdict: the gate's bytes or None (every
        message has an aircraft); geom_delta: one int32 per message, INT32_MIN = not valid.  -> (stream bytes, deferred[] records,
        the number of messages outside the printable domain)."""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        n = len(msgs)

        def arr(a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            assert len(a) == n
            return a
        fields, positions = arr(fields, FIELDS_DTYPE), arr(positions, POSITION_DTYPE)
        verdict, geom_delta = arr(verdict, np.uint8), arr(geom_delta, np.int32)
        cap = n * SBS_LINE_MAX + 64
        out = np.empty(cap, dtype=np.uint8)
        dcap = int(deferred_cap if deferred_cap is not None else (n if verdict is not None else 0))
        deferred = np.zeros(max(dcap, 1), dtype=DEFERRED_DTYPE)
        nb, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if a is not None else None                                     # noqa: E731
        a = SbsArgs(C.sizeof(SbsArgs), SBS_USE_GNSS if use_gnss else 0, msgs.ctypes.data, ptr(fields), ptr(positions), ptr(verdict), ptr(geom_delta),
                    n, int(now_ms), int(override_squawk), out.ctypes.data, cap, C.pointer(nb), deferred.ctypes.data, dcap, C.pointer(nd), C.pointer(ns))
        self._chk(self.lib.mgpu_sbs_encode_ex(self.ctx, C.byref(a)), "mgpu_sbs_encode_ex")
        return out[: nb.value].tobytes(), deferred[: nd.value].copy(), int(ns.value)

    def sbs_encode_device(self, d_msgs_ptr, d_fields_ptr, n, now_ms, d_out_ptr, cap, d_positions_ptr=None, d_verdict_ptr=None, d_geom_delta_ptr=None,
                          use_gnss=False, override_squawk=-1, d_deferred_ptr=None, deferred_cap=0):
        """mgpu_sbs_encode_ex_device: everything in HBM (pointers as ints).  -> (the stream's size in bytes, the number of deferred
        messages, the number of skipped messages)."""
        nb, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        a = SbsArgs(C.sizeof(SbsArgs), SBS_USE_GNSS if use_gnss else 0, d_msgs_ptr, d_fields_ptr, d_positions_ptr, d_verdict_ptr, d_geom_delta_ptr,
                    n, int(now_ms), int(override_squawk), d_out_ptr, cap, C.pointer(nb), d_deferred_ptr, deferred_cap, C.pointer(nd), C.pointer(ns))
        self._chk(self.lib.mgpu_sbs_encode_ex_device(self.ctx, C.byref(a)), "mgpu_sbs_encode_ex_device")
        return int(nb.value), int(nd.value), int(ns.value)

    @staticmethod
    def _dump_host_args(msgs, flags, fields, reduce_forward, receiver_ids, positions, decoded_nic, decoded_rc, show_only):
        """-> (struct mgpu_dump_args over host arrays with the output members empty, the arrays it points into)"""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        n = len(msgs)

        def arr(a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            assert len(a) == n
            return a
        keep = [msgs, arr(fields, FIELDS_DTYPE), arr(reduce_forward, np.uint8), arr(receiver_ids, np.uint64), arr(positions, POSITION_DTYPE),
                arr(decoded_nic, np.uint8), arr(decoded_rc, np.uint32)]
        ptr = lambda a: a.ctypes.data if a is not None else None                                     # noqa: E731
        a = DumpArgs(C.sizeof(DumpArgs), int(flags), *[ptr(k) for k in keep], n, int(show_only))
        return a, keep

    def dump_encode(self, msgs, flags=0, fields=None, reduce_forward=None, receiver_ids=None, positions=None, decoded_nic=None, decoded_rc=None,
                    show_only=0, cap=None, deferred_cap=None):
        """mgpu_dump_encode_ex on host arrays: the decoded-message dumps of a record array, displayModesMessage's bytes
        (include/modes_gpu.h).  flags: DUMP_*; fields: decode_fields' records or None (decoded by the library); the other arrays are
        the host tracker's, None = 0.  -> (stream bytes, deferred[] records — the messages whose RSSI rounding is the host's to settle,
        see dump_format_host — the number of messages outside the printable domain)."""
        a, keep = self._dump_host_args(msgs, flags, fields, reduce_forward, receiver_ids, positions, decoded_nic, decoded_rc, show_only)
        n = len(keep[0])
        cap = int(cap if cap is not None else n * DUMP_MAX + 64)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        dcap = int(deferred_cap if deferred_cap is not None else n)
        deferred = np.zeros(max(dcap, 1), dtype=DEFERRED_DTYPE)
        nb, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        a.out, a.cap, a.bytes, a.deferred, a.deferred_cap, a.ndeferred, a.nskipped = out.ctypes.data, cap, C.pointer(nb), deferred.ctypes.data, dcap, C.pointer(nd), \
            C.pointer(ns)
        self._chk(self.lib.mgpu_dump_encode_ex(self.ctx, C.byref(a)), "mgpu_dump_encode_ex")
        return out[: nb.value].tobytes(), deferred[: nd.value].copy(), int(ns.value)

    def dump_encode_device(self, d_msgs_ptr, d_fields_ptr, n, d_out_ptr, cap, flags=0, d_reduce_forward_ptr=None, d_receiver_ids_ptr=None, d_positions_ptr=None,
                           d_decoded_nic_ptr=None, d_decoded_rc_ptr=None, show_only=0, d_deferred_ptr=None, deferred_cap=0):
        """mgpu_dump_encode_ex_device: everything in HBM (pointers as ints).  -> (the stream's size in bytes, the number of deferred
        messages, the number of skipped messages)."""
        nb, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        a = DumpArgs(C.sizeof(DumpArgs), int(flags), d_msgs_ptr, d_fields_ptr, d_reduce_forward_ptr, d_receiver_ids_ptr, d_positions_ptr, d_decoded_nic_ptr,
                     d_decoded_rc_ptr, n, int(show_only), d_out_ptr, cap, C.pointer(nb), d_deferred_ptr, deferred_cap, C.pointer(nd), C.pointer(ns))
        self._chk(self.lib.mgpu_dump_encode_ex_device(self.ctx, C.byref(a)), "mgpu_dump_encode_ex_device")
        return int(nb.value), int(nd.value), int(ns.value)

    def dump_format_host(self, index, msgs, fields, flags=0, reduce_forward=None, receiver_ids=None, positions=None, decoded_nic=None, decoded_rc=None,
                         show_only=0):
        """mgpu_dump_format_host: the dump of message `index` formatted on the host (the host's log10) — the text to splice in at a
        deferred entry's offset.  -> bytes (empty: the message gets no dump in this mode)."""
        a, keep = self._dump_host_args(msgs, flags, fields, reduce_forward, receiver_ids, positions, decoded_nic, decoded_rc, show_only)
        text = np.empty(DUMP_MAX, dtype=np.uint8)
        k = self.lib.mgpu_dump_format_host(C.byref(a), int(index), text.ctypes.data, DUMP_MAX)
        if k < 0:
            raise MgpuError(f"mgpu_dump_format_host: {k}")
        return text[:k].tobytes()

    def asterix_encode(self, msgs, now_ms, fields=None, positions=None, verdict=None, ids=None, ac_baro_alt=None, ac_category=None, remote=False,
                       deferred_cap=None):
        """mgpu_asterix_encode_ex on host arrays: the ASTERIX CAT021 target reports of a record array (include/modes_gpu.h).  fields,
        positions, verdict as in sbs_encode (the verdict decides as for the raw lines); ids: merge_by_time's receiver ids or None;
        ac_baro_alt (int32) / ac_category (uint8): the aircraft's state per message, None = a fresh aircraft's zeros.
        -> (stream bytes, deferred[] records, the number of messages outside the domain)."""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        n = len(msgs)

        def arr(a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            assert len(a) == n
            return a
        fields, positions, verdict = arr(fields, FIELDS_DTYPE), arr(positions, POSITION_DTYPE), arr(verdict, np.uint8)
        ids, ac_baro_alt, ac_category = arr(ids, np.uint64), arr(ac_baro_alt, np.int32), arr(ac_category, np.uint8)
        cap = n * ASTERIX_RECORD_MAX + 64
        out = np.empty(cap, dtype=np.uint8)
        dcap = int(deferred_cap if deferred_cap is not None else (n if verdict is not None else 0))
        deferred = np.zeros(max(dcap, 1), dtype=DEFERRED_DTYPE)
        nb, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if a is not None else None                                     # noqa: E731
        a = AsterixArgs(C.sizeof(AsterixArgs), ASTERIX_REMOTE if remote else 0, msgs.ctypes.data, ptr(fields), ptr(positions), ptr(verdict), ptr(ids),
                        ptr(ac_baro_alt), ptr(ac_category), n, int(now_ms), out.ctypes.data, cap, C.pointer(nb), deferred.ctypes.data, dcap,
                        C.pointer(nd), C.pointer(ns))
        self._chk(self.lib.mgpu_asterix_encode_ex(self.ctx, C.byref(a)), "mgpu_asterix_encode_ex")
        return out[: nb.value].tobytes(), deferred[: nd.value].copy(), int(ns.value)

    def asterix_encode_device(self, d_msgs_ptr, d_fields_ptr, n, now_ms, d_out_ptr, cap, d_positions_ptr=None, d_verdict_ptr=None, d_ids_ptr=None,
                              d_ac_baro_alt_ptr=None, d_ac_category_ptr=None, remote=False, d_deferred_ptr=None, deferred_cap=0):
        """mgpu_asterix_encode_ex_device: everything in HBM (pointers as ints).  -> (the stream's size in bytes, the number of deferred
        messages, the number of skipped messages)."""
        nb, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        a = AsterixArgs(C.sizeof(AsterixArgs), ASTERIX_REMOTE if remote else 0, d_msgs_ptr, d_fields_ptr, d_positions_ptr, d_verdict_ptr, d_ids_ptr,
                        d_ac_baro_alt_ptr, d_ac_category_ptr, n, int(now_ms), d_out_ptr, cap, C.pointer(nb), d_deferred_ptr, deferred_cap,
                        C.pointer(nd), C.pointer(ns))
        self._chk(self.lib.mgpu_asterix_encode_ex_device(self.ctx, C.byref(a)), "mgpu_asterix_encode_ex_device")
        return int(nb.value), int(nd.value), int(ns.value)

    @staticmethod
    def _raw_flags(mlat, net_rule, verbatim):
        return (RAW_MLAT if mlat else 0) | (RAW_NET_RULE if net_rule else 0) | (RAW_VERBATIM if verbatim else 0)

    def raw_encode(self, msgs, mlat=False, verdict=None, net_rule=False, verbatim=False, deferred_cap=None):
        """mgpu_raw_encode_ex on host arrays: the AVR raw lines ('*...;' or, with mlat, '@' + 12 timestamp digits) of a record array.
        verdict / net_rule / verbatim as in beast_encode_ex.  -> (stream bytes, deferred[] records)."""
        msgs = np.ascontiguousarray(msgs)
        assert msgs.dtype == MSG_DTYPE
        n = len(msgs)
        if verdict is not None:
            verdict = np.ascontiguousarray(verdict, dtype=np.uint8)
            assert len(verdict) == n
        cap = n * RAW_LINE_MAX + 64
        out = np.empty(cap, dtype=np.uint8)
        dcap = int(deferred_cap if deferred_cap is not None else (n if verdict is not None else 0))
        deferred = np.zeros(max(dcap, 1), dtype=DEFERRED_DTYPE)
        nb, nd = C.c_uint64(0), C.c_uint64(0)
        a = RawArgs(C.sizeof(RawArgs), self._raw_flags(mlat, net_rule, verbatim), msgs.ctypes.data, verdict.ctypes.data if verdict is not None else None,
                    n, out.ctypes.data, cap, C.pointer(nb), deferred.ctypes.data, dcap, C.pointer(nd))
        self._chk(self.lib.mgpu_raw_encode_ex(self.ctx, C.byref(a)), "mgpu_raw_encode_ex")
        return out[: nb.value].tobytes(), deferred[: nd.value].copy()

    def raw_encode_device(self, d_msgs_ptr, n, d_out_ptr, cap, mlat=False, d_verdict_ptr=None, net_rule=False, verbatim=False, d_deferred_ptr=None,
                          deferred_cap=0):
        """mgpu_raw_encode_ex_device: everything in HBM (pointers as ints).  -> (the stream's size in bytes, the number of deferred messages)."""
        nb, nd = C.c_uint64(0), C.c_uint64(0)
        a = RawArgs(C.sizeof(RawArgs), self._raw_flags(mlat, net_rule, verbatim), d_msgs_ptr, d_verdict_ptr, n, d_out_ptr, cap, C.pointer(nb),
                    d_deferred_ptr, deferred_cap, C.pointer(nd))
        self._chk(self.lib.mgpu_raw_encode_ex_device(self.ctx, C.byref(a)), "mgpu_raw_encode_ex_device")
        return int(nb.value), int(nd.value)

    def snip(self, iq, level, quiet_run=0, pass_samples=0):
        """mgpu_snip on a host array of UC8 bytes (`readsb --snip level`): every stretch of quiet samples cut down to its first 32.  A
        trailing odd byte is dropped.  quiet_run: the counter a stream's earlier calls left (0: a fresh stream); pass_samples: samples
        staged per pass (0: the library's default).  -> (the kept bytes as a uint8 array, the counter for the stream's next call)."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1)
        n = iq.size // 2
        out = np.empty(2 * n, dtype=np.uint8)
        nout, run = C.c_uint64(0), C.c_uint64(int(quiet_run))
        a = SnipArgs(C.sizeof(SnipArgs), int(level), iq.ctypes.data, n, out.ctypes.data, n, C.pointer(nout), C.pointer(run), int(pass_samples))
        self._chk(self.lib.mgpu_snip(self.ctx, C.byref(a)), "mgpu_snip")
        return out[: 2 * nout.value].copy(), int(run.value)

    def snip_device(self, d_iq_ptr, nsamples, level, d_out_ptr, cap_samples, quiet_run=0):
        """mgpu_snip_device: samples and output in HBM (pointers as ints; the samples 16-byte aligned, the output 2-byte aligned).
        -> (samples kept, the counter for the stream's next call)."""
        nout, run = C.c_uint64(0), C.c_uint64(int(quiet_run))
        a = SnipArgs(C.sizeof(SnipArgs), int(level), d_iq_ptr, int(nsamples), d_out_ptr, int(cap_samples), C.pointer(nout), C.pointer(run), 0)
        self._chk(self.lib.mgpu_snip_device(self.ctx, C.byref(a)), "mgpu_snip_device")
        return int(nout.value), int(run.value)

    def uat_encode(self, text, now_ms=0, settle=True, pass_bytes=0):
        """mgpu_uat_encode on a host byte string of dump978 lines (`--net-uat-in-port`): every downlink line to its DF18 extended
        squitters as AVR lines, the reference's uat2esnt byte for byte.  settle: the lines the device defers (a signal value outside
        dump978's %.1f form, a line longer than 256 bytes) are formatted on the host (mgpu_uat_format_host) and put where they belong;
        otherwise they are left out and listed.  -> dict(text, msgs, sig, line_of, consumed, nlines, nshort, deferred)."""
        buf = np.frombuffer(bytes(text), dtype=np.uint8)
        most = buf.size * 4 // 37 + 4                       # at most 4 frames per 37 bytes of text (uat_format.h)
        out = np.empty(most * UAT_FRAME_TEXT, dtype=np.uint8)
        msgs, sig, line_of = np.zeros(most, dtype=MSG_DTYPE), np.empty(most, dtype=np.uint8), np.empty(most, dtype=np.uint64)
        deferred = np.empty(buf.size // 14 + 1, dtype=np.uint64)     # a deferred line has 14 bytes at least
        c = [C.c_uint64(0) for _ in range(6)]
        a = UatArgs(C.sizeof(UatArgs), 0, buf.ctypes.data if buf.size else None, buf.size, out.ctypes.data, out.size, msgs.ctypes.data, sig.ctypes.data,
                    line_of.ctypes.data, most, deferred.ctypes.data, deferred.size, int(now_ms), *[C.pointer(x) for x in c], int(pass_bytes))
        self._chk(self.lib.mgpu_uat_encode(self.ctx, C.byref(a)), "mgpu_uat_encode")
        nbytes, consumed, nlines, nframes, nshort, ndef = (int(x.value) for x in c)
        res = dict(text=out[:nbytes].tobytes(), msgs=msgs[:nframes].copy(), sig=sig[:nframes].copy(), line_of=line_of[:nframes].copy(), consumed=consumed,
                   nlines=nlines, nshort=nshort, deferred=deferred[:ndef].copy())
        if settle and ndef:
            parts, recs, sigs, lines, at = [], [], [], [], 0
            line_buf, rec_buf, sig_buf = np.empty(4 * UAT_FRAME_TEXT, dtype=np.uint8), np.zeros(4, dtype=MSG_DTYPE), C.c_uint8(0)

            def take(upto):
                nonlocal at
                parts.append(res["text"][at * UAT_FRAME_TEXT: upto * UAT_FRAME_TEXT])
                recs.append(res["msgs"][at:upto]); sigs.append(res["sig"][at:upto]); lines.append(res["line_of"][at:upto])
                at = upto
            for index in res["deferred"].tolist():
                take(int(np.searchsorted(res["line_of"], index)))
                n = int(self.lib.mgpu_uat_format_host(C.byref(a), index, line_buf.ctypes.data, line_buf.size, rec_buf.ctypes.data, C.addressof(sig_buf)))
                if n < 0:
                    raise MgpuError(f"mgpu_uat_format_host failed ({n})")
                k = n // UAT_FRAME_TEXT
                parts.append(line_buf[:n].tobytes())
                recs.append(rec_buf[:k].copy()); sigs.append(np.full(k, sig_buf.value, dtype=np.uint8)); lines.append(np.full(k, index, dtype=np.uint64))
            take(nframes)
            res.update(text=b"".join(parts), msgs=np.concatenate(recs), sig=np.concatenate(sigs), line_of=np.concatenate(lines))
        return res

    def sbs_decode(self, text, source="sbs", now_ms=0, settle=True, pass_bytes=0):
        """mgpu_sbs_decode on a host byte string of BaseStation lines (`--net-sbs-in-port`, the MLAT, JAERO and PRIO ports): one record
        per valid line, the reference's decodeSbsLine member for member.  source: "sbs", "mlat", "jaero", "prio" or the reference's
        number.  settle: the lines the device defers (a number outside the plain forms) are parsed on the host (mgpu_sbs_parse_host)
        and their records put where they belong; otherwise they are left out and listed.
        -> dict(recs, line_of, consumed, nlines, ninvalid, deferred)."""
        buf = np.frombuffer(bytes(text), dtype=np.uint8)
        most = buf.size // 21 + 1                           # a record needs 20 bytes and a terminator (sbs_in_format.h)
        recs, line_of, deferred = np.zeros(most, dtype=SBS_REC_DTYPE), np.empty(most, dtype=np.uint64), np.empty(most, dtype=np.uint64)
        c = [C.c_uint64(0) for _ in range(5)]
        a = SbsInArgs(C.sizeof(SbsInArgs), SBS_SOURCES.get(source, source), buf.ctypes.data if buf.size else None, buf.size, int(now_ms), recs.ctypes.data,
                      line_of.ctypes.data, most, deferred.ctypes.data, most, *[C.pointer(x) for x in c], int(pass_bytes))
        self._chk(self.lib.mgpu_sbs_decode(self.ctx, C.byref(a)), "mgpu_sbs_decode")
        consumed, nlines, nrecs, ninvalid, ndef = (int(x.value) for x in c)
        res = dict(recs=recs[:nrecs].copy(), line_of=line_of[:nrecs].copy(), consumed=consumed, nlines=nlines, ninvalid=ninvalid, deferred=deferred[:ndef].copy())
        if settle and ndef:
            one = np.zeros(1, dtype=SBS_REC_DTYPE)
            extra_recs, extra_lines = [], []
            for index in res["deferred"].tolist():
                rc = int(self.lib.mgpu_sbs_parse_host(C.byref(a), index, one.ctypes.data))
                if rc < 0:
                    raise MgpuError(f"mgpu_sbs_parse_host failed ({rc})")
                if rc:
                    extra_recs.append(one.copy()); extra_lines.append(index)
            if extra_lines:
                where = np.searchsorted(res["line_of"], np.array(extra_lines, dtype=np.uint64))
                res.update(recs=np.insert(res["recs"], where, np.concatenate(extra_recs)), line_of=np.insert(res["line_of"], where, np.array(extra_lines, dtype=np.uint64)))
        return res

    def raw_decode(self, text, now_ms=0, pass_bytes=0):
        """mgpu_raw_decode on a host byte string of AVR lines (`--net-ri-port`): the messages the reference's decodeHexMessage accepts,
        in line order, the ICAO filter's answers as they stand at every line; the context's filter learns the stream's clean DF17 /
        DF11 addresses, and the demodulator on this context sees them.
        -> dict(msgs, line_of, signal_level, line_class, consumed, nlines, counters)."""
        buf = np.frombuffer(bytes(text), dtype=np.uint8)
        most = buf.size // 6 + 1                            # a frame line needs 5 bytes and a terminator (raw_in_format.h)
        msgs, line_of, signal = np.zeros(most, dtype=MSG_DTYPE), np.empty(most, dtype=np.uint64), np.empty(most, dtype=np.float64)
        cls = np.zeros(buf.size + 1, dtype=np.uint8)
        c = [C.c_uint64(0) for _ in range(3)]
        cn = RawInCounters()
        a = RawInArgs(C.sizeof(RawInArgs), 0, buf.ctypes.data if buf.size else None, buf.size, int(now_ms), msgs.ctypes.data, line_of.ctypes.data, signal.ctypes.data, most,
                      cls.ctypes.data, cls.size, *[C.pointer(x) for x in c], C.pointer(cn), int(pass_bytes))
        self._chk(self.lib.mgpu_raw_decode(self.ctx, C.byref(a)), "mgpu_raw_decode")
        consumed, nlines, n = (int(x.value) for x in c)
        counters = dict(remote_received_modes=int(cn.remote_received_modes), remote_received_modeac=int(cn.remote_received_modeac),
                        remote_rejected_unknown_icao=int(cn.remote_rejected_unknown_icao), remote_rejected_bad=int(cn.remote_rejected_bad),
                        remote_accepted=[int(x) for x in cn.remote_accepted])
        return dict(msgs=msgs[:n].copy(), line_of=line_of[:n].copy(), signal_level=signal[:n].copy(), line_class=cls[:nlines].copy(), consumed=consumed, nlines=nlines,
                    counters=counters)

    def beast_decode(self, data, now_ms=0, receiver_id=0, net_ingest=False, pass_bytes=0):
        """mgpu_beast_decode on a host byte string of beast binary (`--net-bi-port`): one readBeast with decodeBinMessage behind it —
        the accepted messages in stream order, each with the receiver id in force at its frame, the ICAO filter's answers as they
        stand at every frame; the context's filter learns the stream's clean DF17 / DF11 addresses.
        -> dict(msgs, receiver_id, signal_level, frame_of, frame_class, frame_off, consumed, nframes, stop, stop_off, receiver_id_out, counters)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        most, mostf = buf.size // 11 + 1, buf.size // 5 + 1   # a message needs 11 bytes, a handler call 5 (beast_in_format.h)
        msgs, ids = np.zeros(most, dtype=MSG_DTYPE), np.zeros(most, dtype=np.uint64)
        signal, frame_of = np.empty(most, dtype=np.float64), np.empty(most, dtype=np.uint64)
        cls, off = np.zeros(mostf, dtype=np.uint8), np.zeros(mostf, dtype=np.uint64)
        c = [C.c_uint64(0) for _ in range(5)]
        stop = C.c_uint32(0)
        cn = BeastInCounters()
        a = BeastInArgs(C.sizeof(BeastInArgs), 0, buf.ctypes.data if buf.size else None, buf.size, int(now_ms), int(receiver_id), int(bool(net_ingest)), 0,
                        msgs.ctypes.data, ids.ctypes.data, signal.ctypes.data, frame_of.ctypes.data, most, cls.ctypes.data, off.ctypes.data, mostf,
                        C.pointer(c[0]), C.pointer(c[1]), C.pointer(c[2]), C.pointer(stop), C.pointer(c[3]), C.pointer(c[4]), C.pointer(cn), int(pass_bytes))
        self._chk(self.lib.mgpu_beast_decode(self.ctx, C.byref(a)), "mgpu_beast_decode")
        consumed, nframes, n, stop_off, id_out = (int(x.value) for x in c)
        return dict(msgs=msgs[:n].copy(), receiver_id=ids[:n].copy(), signal_level=signal[:n].copy(), frame_of=frame_of[:n].copy(), frame_class=cls[:nframes].copy(),
                    frame_off=off[:nframes].copy(), consumed=consumed, nframes=nframes, stop=int(stop.value), stop_off=stop_off, receiver_id_out=id_out,
                    counters=beast_in_counters_dict(cn))

    def pf_decode(self, data, now_ms=0, pass_bytes=0):
        """mgpu_pf_decode on a host byte string of the Planefinder binary feed (`--net-pfms-in-port`): one readPlanefinder with
        decodePfMessage behind it — the accepted messages in stream order, the ICAO filter's answers as they stand at every frame; the
        context's filter learns the stream's clean DF17 / DF11 addresses.
        -> dict(msgs, signal_level, frame_of, frame_class, frame_off, consumed, nframes, counters)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        most = buf.size // 4 + 1                            # a handler call needs 4 bytes (pf_in_format.h)
        msgs, signal, frame_of = np.zeros(most, dtype=MSG_DTYPE), np.empty(most, dtype=np.float64), np.empty(most, dtype=np.uint64)
        cls, off = np.zeros(most, dtype=np.uint8), np.zeros(most, dtype=np.uint64)
        c = [C.c_uint64(0) for _ in range(3)]
        cn = PfInCounters()
        a = PfInArgs(C.sizeof(PfInArgs), 0, buf.ctypes.data if buf.size else None, buf.size, int(now_ms), msgs.ctypes.data, signal.ctypes.data, frame_of.ctypes.data, most,
                     cls.ctypes.data, off.ctypes.data, most, C.pointer(c[0]), C.pointer(c[1]), C.pointer(c[2]), C.pointer(cn), int(pass_bytes))
        self._chk(self.lib.mgpu_pf_decode(self.ctx, C.byref(a)), "mgpu_pf_decode")
        consumed, nframes, n = (int(x.value) for x in c)
        return dict(msgs=msgs[:n].copy(), signal_level=signal[:n].copy(), frame_of=frame_of[:n].copy(), frame_class=cls[:nframes].copy(), frame_off=off[:nframes].copy(),
                    consumed=consumed, nframes=nframes, counters=pf_in_counters_dict(cn))

    def asterix_decode(self, data, source=1, now_ms=0, pass_bytes=0):
        """mgpu_asterix_decode on a host byte string of ASTERIX records (`--net-asterix-in-port`): one record per category-21 frame
        with an address, the reference's decodeAsterixMessage member for member.  source: the reference's datasource_t (1:
        SOURCE_INDIRECT).  Two calls: the first counts, the second fills arrays of that size.
        -> dict(recs, frame_of, consumed, nframes, nother, nundefined, stop)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        c = [C.c_uint64(0) for _ in range(5)]
        stop = C.c_uint32(0)

        def call(recs, frame_of, cap):
            a = AsterixInArgs(C.sizeof(AsterixInArgs), int(source), buf.ctypes.data if buf.size else None, buf.size, int(now_ms), recs, frame_of, cap, int(pass_bytes),
                              C.pointer(c[0]), C.pointer(c[1]), C.pointer(c[2]), C.pointer(stop), C.pointer(c[3]), C.pointer(c[4]))
            return int(self.lib.mgpu_asterix_decode(self.ctx, C.byref(a)))
        rc = call(None, None, 0)
        if rc not in (0, -5):                               # MGPU_E_OVERFLOW: *nrecs is what is needed
            self._chk(rc, "mgpu_asterix_decode")
        n = int(c[2].value)
        recs, frame_of = np.zeros(n, dtype=ASTERIX_REC_DTYPE), np.zeros(n, dtype=np.uint64)
        if n:
            self._chk(call(recs.ctypes.data, frame_of.ctypes.data, n), "mgpu_asterix_decode")
        return dict(recs=recs, frame_of=frame_of, consumed=int(c[0].value), nframes=int(c[1].value), nother=int(c[3].value), nundefined=int(c[4].value),
                    stop=int(stop.value))

    def merge_by_time(self, lists, ids=None, verdicts=None):
        """mgpu_merge_by_time on host arrays: the receivers' lists merged by timestamp on the GPU, equal stamps in input order —
        gather.merge_by_timestamp's result.  ids: one receiver id per list, verdicts: one byte array per list (or None).
        -> (merged records, permutation into the concatenation, id per record, verdict per record or None)."""
        lists = [np.ascontiguousarray(m) for m in lists]
        assert all(m.dtype == MSG_DTYPE for m in lists)
        nseg, n = len(lists), sum(len(m) for m in lists)
        ptrs = (C.c_void_p * max(nseg, 1))(*[m.ctypes.data for m in lists])
        counts = np.array([len(m) for m in lists], dtype=np.uint64)
        seg_ids = np.ascontiguousarray(ids if ids is not None else np.zeros(nseg), dtype=np.uint64)
        assert len(seg_ids) == nseg
        vptrs = None
        if verdicts is not None:
            verdicts = [np.ascontiguousarray(v, dtype=np.uint8) for v in verdicts]
            assert [len(v) for v in verdicts] == [len(m) for m in lists]
            vptrs = (C.c_void_p * max(nseg, 1))(*[v.ctypes.data for v in verdicts])
        out, perm, oid = np.empty(n, dtype=MSG_DTYPE), np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
        vout = np.empty(n, dtype=np.uint8) if verdicts is not None else None
        self._chk(self.lib.mgpu_merge_by_time(self.ctx, C.cast(ptrs, C.c_void_p), C.c_void_p(counts.ctypes.data), nseg, C.c_void_p(seg_ids.ctypes.data),
                                              C.cast(vptrs, C.c_void_p) if vptrs is not None else None, C.c_void_p(out.ctypes.data),
                                              C.c_void_p(perm.ctypes.data), C.c_void_p(oid.ctypes.data),
                                              C.c_void_p(vout.ctypes.data) if vout is not None else None), "mgpu_merge_by_time")
        return out, perm, oid, vout

    def merge_by_time_device(self, d_segment_ptrs, counts, d_out_ptr, ids=None, d_verdict_ptrs=None, d_perm_ptr=None, d_ids_ptr=None, d_verdict_out_ptr=None):
        """mgpu_merge_by_time_device: d_segment_ptrs / counts = one device pointer (int) and one length per list; the merged records go
        to d_out_ptr, optionally the permutation / ids (u64 each) / verdict bytes to the other pointers.  -> the number of records."""
        nseg = len(counts)
        assert len(d_segment_ptrs) == nseg
        ptrs = (C.c_void_p * max(nseg, 1))(*[int(p) if p else None for p in d_segment_ptrs])
        cnt = np.array([int(k) for k in counts], dtype=np.uint64)
        seg_ids = np.ascontiguousarray(ids if ids is not None else np.zeros(nseg), dtype=np.uint64)
        assert len(seg_ids) == nseg
        vptrs = (C.c_void_p * max(nseg, 1))(*[int(p) if p else None for p in d_verdict_ptrs]) if d_verdict_ptrs is not None else None
        self._chk(self.lib.mgpu_merge_by_time_device(self.ctx, C.cast(ptrs, C.c_void_p), C.c_void_p(cnt.ctypes.data), nseg, C.c_void_p(seg_ids.ctypes.data),
                                                     C.cast(vptrs, C.c_void_p) if vptrs is not None else None, C.c_void_p(d_out_ptr), C.c_void_p(d_perm_ptr),
                                                     C.c_void_p(d_ids_ptr), C.c_void_p(d_verdict_out_ptr)), "mgpu_merge_by_time_device")
        return int(cnt.sum())

    def merge_last_passes(self):
        """8-bit digit passes the last merge took (those up to the highest bit in which its stamps differed)."""
        return int(self.lib.mgpu_merge_last_passes(self.ctx))

    def beast_encode_device(self, d_msgs_ptr, n, d_out_ptr, cap):
        """Same on device pointers (ints, e.g. torch tensor.data_ptr()); returns the stream's size in bytes."""
        nb = C.c_uint64(0)
        self._chk(self.lib.mgpu_beast_encode_device(self.ctx, C.c_void_p(d_msgs_ptr), n, C.c_void_p(d_out_ptr), cap, C.byref(nb)), "mgpu_beast_encode_device")
        return int(nb.value)

    def beast_encode_gated_device(self, d_msgs_ptr, d_verdict_ptr, n, d_out_ptr, cap, d_deferred_ptr, deferred_cap, net_rule=False):
        """mgpu_beast_encode_gated_device: the caller's verdict bytes applied to records in HBM, stream and deferred[] list written to
        HBM; returns (the stream's size in bytes, the number of deferred messages)."""
        nb, nd = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.mgpu_beast_encode_gated_device(self.ctx, C.c_void_p(d_msgs_ptr), C.c_void_p(d_verdict_ptr), C.c_uint64(n),
                                                          C.c_uint32(1 if net_rule else 0), C.c_void_p(d_out_ptr), C.c_uint64(cap), C.byref(nb),
                                                          C.c_void_p(d_deferred_ptr), C.c_uint64(deferred_cap), C.byref(nd)),
                  "mgpu_beast_encode_gated_device")
        return int(nb.value), int(nd.value)

    def host_cpus(self):
        """CPUs the context's host threads are pinned to (empty list: not pinned)."""
        buf = (C.c_int32 * 64)()
        n = int(self.lib.mgpu_host_cpus(self.ctx, buf, 64))
        return [int(buf[i]) for i in range(max(0, min(n, 64)))]

    def keep_other_threads_away(self, confine_to_own_l3=False):
        """Move every thread of this process that is not one of the context's pinned threads off the pinned cores and
        their SMT siblings (the application side of mgpu_host_cpus' advice; Linux only, best effort).
        confine_to_own_l3=True (several ranks on one node): the other threads go to the free SMT siblings of the
        context's own L3 group instead, so that they cannot wander onto another rank's pipeline cores either."""
        cpus = self.host_cpus()
        if not cpus:
            return 0

        def cpulist(path):
            out = set()
            try:
                for part in open(path).read().strip().split(","):
                    lo, _, hi = part.partition("-")
                    out.update(range(int(lo), int(hi or lo) + 1))
            except (OSError, ValueError):
                pass
            return out

        siblings, l3 = set(), set()
        for c in cpus:
            siblings |= cpulist(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list") or {c}
            l3 |= cpulist(f"/sys/devices/system/cpu/cpu{c}/cache/index3/shared_cpu_list")
        moved = 0
        for tid in os.listdir("/proc/self/task"):
            try:
                cur = os.sched_getaffinity(int(tid))
                if len(cur) == 1 and next(iter(cur)) in cpus:
                    continue                       # one of the pipeline's own threads
                target = ((l3 - set(cpus)) & cur) if confine_to_own_l3 else (cur - siblings)
                if target and target != cur:
                    os.sched_setaffinity(int(tid), target)
                    moved += 1
            except OSError:
                pass
        return moved

    def host_register(self, arr):
        """Page-lock a numpy array the caller keeps feeding from (mgpu_host_register)."""
        self._chk(self.lib.mgpu_host_register(self.ctx, C.c_void_p(arr.ctypes.data), C.c_uint64(arr.nbytes)), "mgpu_host_register")

    def host_unregister(self, arr):
        self._chk(self.lib.mgpu_host_unregister(self.ctx, C.c_void_p(arr.ctypes.data)), "mgpu_host_unregister")

    def collect(self, reuse=False, out=None):
        """Drain the decoded messages (stream order) and read the counters.

        reuse=True returns a view of a buffer the Demodulator keeps and overwrites on the next
        collect(reuse=True): a steady consumer then pays one copy and no page faults per call.
        out=<record array> collects into the caller's buffer (e.g. pinned staging memory).
        """
        n = int(self.lib.mgpu_pending_messages(self.ctx))
        if out is not None:
            if out.dtype != MSG_DTYPE or not out.flags["C_CONTIGUOUS"] or out.size < n:
                raise ValueError("collect(out=...): need a contiguous mgpu_msg array with room for %d records" % n)
        elif reuse:
            if self._collect_buf is None or self._collect_buf.size < n:
                self._collect_buf = np.empty(max(n, 1024) * 5 // 4, dtype=MSG_DTYPE)
            out = self._collect_buf
        else:
            out = np.empty(n, dtype=MSG_DTYPE)
        got = C.c_uint64(0)
        cnt = Counters()
        self._chk(self.lib.mgpu_collect(self.ctx, out.ctypes.data, n, C.byref(got), C.byref(cnt)), "mgpu_collect")
        return out[: got.value], cnt.as_dict()

    def host_alloc(self, nbytes):
        """Page-locked host memory on the device's NUMA node as a uint8 numpy array (mgpu_host_alloc); host_free(arr) releases it."""
        p = self.lib.mgpu_host_alloc(self.ctx, int(nbytes))
        if not p:
            raise MgpuError("mgpu_host_alloc failed")
        arr = np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(p))
        self._host_allocs = getattr(self, "_host_allocs", {})
        self._host_allocs[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_host_allocs", {}).pop(arr.ctypes.data, None)
        if p:
            self.lib.mgpu_host_free(self.ctx, p)

    def set_deferred(self, on=True):
        """mgpu_set_deferred: feeds return once enqueued; the loop is feed(k+1); collect_feed(k)."""
        self._chk(self.lib.mgpu_set_deferred(self.ctx, 1 if on else 0), "mgpu_set_deferred")

    def set_device_messages(self, on=True):
        """mgpu_set_device_messages (deferred mode): the messages of a feed are built on the GPU and stay there (True / 1), or are
        stored by the GPU into the page-locked array set_message_buffer named for the feed (2)."""
        self._chk(self.lib.mgpu_set_device_messages(self.ctx, int(on)), "mgpu_set_device_messages")

    def set_device_message_buffer(self, dptr, capacity):
        """mgpu_set_device_message_buffer: the next feed's records go to device address dptr (capacity records); None: the library's list."""
        self._chk(self.lib.mgpu_set_device_message_buffer(self.ctx, C.c_void_p(dptr) if dptr else None, C.c_uint64(capacity if dptr else 0)),
                  "mgpu_set_device_message_buffer")

    def collect_feed_device(self, want_counters=False):
        """Device-messages mode: wait for the oldest uncollected feed; returns (device pointer of its mgpu_msg records, count,
        counters or None).  The pointer stays valid until three more feeds have been started."""
        ptr, n = C.c_void_p(), C.c_uint64(0)
        cnt = Counters() if want_counters else None
        self._chk(self.lib.mgpu_collect_device(self.ctx, C.byref(ptr), C.byref(n), C.byref(cnt) if cnt is not None else None),
                  "mgpu_collect_device")
        return int(ptr.value or 0), int(n.value), (cnt.as_dict() if cnt is not None else None)

    def collect_feed(self, out, want_counters=False):
        """Deferred mode: wait for the oldest uncollected feed and take its messages into `out` (a contiguous mgpu_msg array,
        possibly the one named by set_message_buffer for that feed: then nothing is copied).  want_counters=True also drains
        everything in flight and returns the settled counters."""
        if out.dtype != MSG_DTYPE or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("collect_feed(out): need a contiguous mgpu_msg array")
        got = C.c_uint64(0)
        cnt = Counters() if want_counters else None
        self._chk(self.lib.mgpu_collect(self.ctx, out.ctypes.data, out.size, C.byref(got), C.byref(cnt) if cnt is not None else None),
                  "mgpu_collect")
        return out[: got.value], (cnt.as_dict() if cnt is not None else None)

    def last_magnitudes(self, n):
        """mgpu_debug_last_magnitudes: the first n magnitudes of the chunk the pipeline demodulated last, out of HBM."""
        out = np.empty(int(n), dtype=np.uint16)
        self._chk(self.lib.mgpu_debug_last_magnitudes(self.ctx, out.ctypes.data, int(n)), "mgpu_debug_last_magnitudes")
        return out

    def device_walk_stats(self):
        """mgpu_debug_device_walk: what the walk on the device (MGPU_DEVICE_WALK) did so far."""
        out = (C.c_uint64 * 8)()
        self._chk(self.lib.mgpu_debug_device_walk(self.ctx, out), "mgpu_debug_device_walk")
        keys = ("chunks", "device", "unsettled", "premises_failed", "not_modelled", "walks", "differences")
        return dict(zip(keys, [int(v) for v in out]))

    def event_bracket_us(self):
        """mgpu_event_bracket_us: what a pair of timing events around one kernel reports beyond the kernel itself (us)."""
        v = C.c_float(0)
        self._chk(self.lib.mgpu_event_bracket_us(self.ctx, C.byref(v)), "mgpu_event_bracket_us")
        return float(v.value)

    def timing(self):
        t = Timing()
        self._chk(self.lib.mgpu_last_timing(self.ctx, C.byref(t)), "mgpu_last_timing")
        return t.as_dict()

    def convert(self, iq):
        """iq_convert_fn: returns (mag u16[n], mean_level, mean_power)."""
        iq, n = self._nsamples(iq)
        mag = np.empty(n, dtype=np.uint16)
        ml, mp = C.c_double(), C.c_double()
        self._chk(self.lib.mgpu_convert(self.ctx, iq.ctypes.data, mag.ctypes.data, n, C.byref(ml), C.byref(mp)), "mgpu_convert")
        return mag, ml.value, mp.value

    def demod_mag_buf(self, data, length, sample_timestamp, sys_timestamp, mean_power, dropped=0):
        """demodulate2400(struct mag_buf *): data = u16[326 + length]."""
        data = np.ascontiguousarray(data, dtype=np.uint16)
        assert data.size >= 326 + length
        self._chk(self.lib.mgpu_demod_mag_buf(self.ctx, data.ctypes.data, length, sample_timestamp, sys_timestamp,
                                              float(mean_power), dropped), "mgpu_demod_mag_buf")

    def demod_mag_buf_ac(self, data, length, sample_timestamp, sys_timestamp, mean_level, mean_power, dropped=0):
        """demodulate2400 + demodulate2400AC on one struct mag_buf (cfg.mode_ac)."""
        data = np.ascontiguousarray(data, dtype=np.uint16)
        assert data.size >= 326 + length
        self._chk(self.lib.mgpu_demod_mag_buf_ac(self.ctx, data.ctypes.data, length, sample_timestamp, sys_timestamp,
                                                 float(mean_level), float(mean_power), dropped), "mgpu_demod_mag_buf_ac")

    def demodulate_capture(self, iq, chunk_samples=None):
        """Whole capture: feed in chunks that are multiples of the buffer size, finish, collect."""
        iq, n = self._nsamples(iq)
        bps = _FMT_BYTES[self.fmt]
        chunk = chunk_samples or int(self.cfg.max_samples)
        chunk -= chunk % int(self.cfg.buf_samples)
        assert chunk > 0
        off = 0
        while off < n:
            k = min(chunk, n - off)
            self.feed_iq(iq[off * bps:(off + k) * bps])
            off += k
        self.finish()
        return self.collect()
