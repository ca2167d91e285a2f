"""dabamd -- Python mirror of the MI355X DAB Mode-I path (include/dabgpu.h).

Thin ctypes layer over lib/libdabgpu.so.  The functions mirror the
sdr-j-dab interfaces they replace (names and argument meaning follow the
reference; file:line in each docstring).  There is no CPU fallback: if the
HIP library or a gfx950 device is missing, every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("DABGPU_LIB") or os.path.join(_PKG, "lib", "libdabgpu.so")   # env: A/B of builds (tools/)
SYNTH_PATH = os.path.join(_PKG, "lib", "libdabsynth.so")

TU, TS, TG, TNULL, TF, K, L = 2048, 2552, 504, 2656, 196608, 1536, 76
NSYM = 75
SYMBITS = 2 * K
CIF_BITS = 55296


class DabError(RuntimeError):
    pass


class Subch(C.Structure):
    """audiodata/packetdata subset (dab-constants.h:151-176)."""
    _fields_ = [("startAddr", C.c_int16), ("length", C.c_int16), ("bitRate", C.c_int16),
                ("protLevel", C.c_int16), ("uepFlag", C.c_int16), ("flags", C.c_int16)]


SUBCH_DABPLUS = 1   # Subch.flags: feed the DAB+ superframe layer
SUBCH_RAW = 2       # Subch.flags (msc_deconvolve): no energy dispersal
SUBCH_MP2 = 4       # Subch.flags: feed the MPEG layer II layer (Pipeline.mp2)
SUBCH_AUDIO = 128   # Subch.flags, with SUBCH_MP2: feed the audio output layer (Pipeline.audio)
AUDIO_STATE_BYTES = 32   # DABGPU_AUDIO_STATE_BYTES
TABLE_AUDIO_FIR = 6      # DABGPU_TABLE_AUDIO_FIR: float32 [3, 5]
MP2_STATE_BYTES = 3840   # DABGPU_MP2_STATE_BYTES: a layer II decoder's carried state
MP2_INFO_DTYPE = np.dtype([("status", "<i4"), ("sample_rate", "<i4"), ("frame_bytes", "<i4")])   # dabgpu_mp2_info
SUBCH_PACKET = 8    # Subch.flags: feed the packet-mode data layer (Pipeline.packet)
PKT_GROUP_BYTES = 8216   # DABGPU_PKT_GROUP_BYTES: the default max_group_bytes
PACKET_INFO_DTYPE = np.dtype([("status", "<i2"), ("packets", "<i2"), ("crc_errors", "<i2"), ("groups", "<i2"),
                              ("quality", "<i2"), ("address", "<i2")])                     # dabgpu_packet_info
PACKET_RUN_DTYPE = np.dtype([("n_groups", "<i4"), ("n_bytes", "<i4"), ("state", "<i4"), ("pending_bytes", "<i4")])
DATAGROUP_DTYPE = np.dtype([("cif", "<i4"), ("offset", "<i4"), ("nbytes", "<i4"), ("data_offset", "<i4"),
                            ("data_nbytes", "<i4"), ("flags", "<u2"), ("segmentNumber", "<u2"), ("transportId", "<u2"),
                            ("groupType", "u1"), ("CI", "u1"), ("lengthInd", "u1"), ("reserved", "u1", (3,))])
DG_EXTENSION, DG_CRC, DG_SEGMENT, DG_USER_ACCESS, DG_LAST, DG_TRANSPORT, DG_ACCEPTED, DG_TRUNCATED = (
    1, 2, 4, 8, 16, 32, 64, 128)


def pkt_group_slots(n_frames: int, max_bitrate: int) -> int:
    """DABGPU_PKT_GROUP_SLOTS"""
    return 4 * n_frames * (max_bitrate // 8)


def pkt_arena_bytes(n_frames: int, max_bitrate: int, max_group_bytes: int) -> int:
    """DABGPU_PKT_ARENA_BYTES"""
    return max_group_bytes + 4 * n_frames * (max_bitrate // 8) * 127


SUBCH_MOT = 16      # Subch.flags, with SUBCH_PACKET: feed the entry's groups to the MOT layer (Pipeline.mot)
MOT_BODY_BYTES, MOT_NAME_BYTES, MOT_ENTRIES = 65536, 128, 16
MOT_SLIDE, MOT_EPG, MOT_FILE = 1, 2, 3      # dabgpu_mot_object.kind
MOT_TOO_LARGE, MOT_OVERFLOW = 1, 2
MOT_OBJECT_DTYPE = np.dtype([("group", "<i4"), ("cif", "<i4"), ("offset", "<i4"), ("nbytes", "<i4"),
                             ("transportId", "<u2"), ("contentType", "u1"), ("kind", "u1"), ("contentsubType", "<u2"),
                             ("flags", "<u2"), ("name_len", "<i4"), ("name", "u1", (MOT_NAME_BYTES,))])   # dabgpu_mot_object
MOT_RUN_DTYPE = np.dtype([("n_objects", "<i4"), ("n_bytes", "<i4"), ("malformed", "<i4"), ("bad_segment", "<i4"),
                          ("other_types", "<i4"), ("entries", "<i4"), ("reserved", "<i4", (2,))])          # dabgpu_mot_run


def mot_arena_bytes(group_slots: int, max_body_bytes: int = MOT_BODY_BYTES) -> int:
    """DABGPU_MOT_ARENA_FOR"""
    return (max_body_bytes + 15) // 16 * 16 + group_slots * 144


def mot_state_bytes(max_body_bytes: int = 0) -> int:
    """dabgpu_mot_state_bytes: a motHandler's carried state (all zero: a new one)"""
    return int(lib().dabgpu_mot_state_bytes(int(max_body_bytes)))


def _records(buf: "DevBuf", dtype: np.dtype, shape) -> np.ndarray:
    raw = buf.download(np.uint8, int(np.prod(shape)) * dtype.itemsize)
    return np.frombuffer(raw.tobytes(), dtype=dtype).reshape(shape)


def mot_groups(ctx: "Context", groups: np.ndarray, data: np.ndarray, run: np.ndarray,
               state: Optional[np.ndarray] = None, max_body_bytes: int = 0, out_arena_bytes: Optional[int] = None):
    """motHandler::process_mscGroup in header mode per slot (dabgpu_mot_groups; mot-data.cpp:
    679-728): groups [n_slots, group_slots] DATAGROUP_DTYPE, data [n_slots, arena] uint8 and run
    [n_slots] PACKET_RUN_DTYPE as Pipeline.packet() returns them for one stream; state
    [n_slots, mot_state_bytes(max_body_bytes)] bytes carried from an earlier call (None: new
    motHandlers).  Returns (objects [n_slots, group_slots] MOT_OBJECT_DTYPE -- the first
    mot_run.n_objects of a row --, bytes [n_slots, out_arena] uint8, mot_run [n_slots]
    MOT_RUN_DTYPE, state)."""
    groups = np.ascontiguousarray(groups, dtype=DATAGROUP_DTYPE)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    run = np.ascontiguousarray(run, dtype=PACKET_RUN_DTYPE)
    n, gs = groups.shape
    assert data.shape[0] == n and run.shape == (n,)
    sb = mot_state_bytes(max_body_bytes)
    if sb == 0:                          # a max_body_bytes the library refuses (DABGPU_E_ARG, before it reads or
        sb, state = 16, None             # writes anything): it gets small buffers and says so itself
        out_arena_bytes = 16 if out_arena_bytes is None else out_arena_bytes
    st = np.zeros((n, sb), np.uint8) if state is None else np.ascontiguousarray(state, dtype=np.uint8).reshape(n, sb)
    oa = mot_arena_bytes(gs, max_body_bytes or MOT_BODY_BYTES) if out_arena_bytes is None else int(out_arena_bytes)
    dg, db, dr, ds = ctx.put(groups.view(np.uint8)), ctx.put(data), ctx.put(run.view(np.uint8)), ctx.put(st)
    do = ctx.buf(max(16, n * gs * MOT_OBJECT_DTYPE.itemsize)).zero()
    dby, dmr = ctx.buf(max(16, n * max(oa, 0))).zero(), ctx.buf(max(16, n * MOT_RUN_DTYPE.itemsize))
    try:
        _chk(lib().dabgpu_mot_groups(ctx.h, ds.ptr, n, int(max_body_bytes), dg.ptr, gs, db.ptr, data.shape[1], dr.ptr,
                                     do.ptr, dby.ptr, oa, dmr.ptr), "dabgpu_mot_groups")
        ctx.sync()
        return (_records(do, MOT_OBJECT_DTYPE, (n, gs)), dby.download(np.uint8, (n, oa)),
                _records(dmr, MOT_RUN_DTYPE, (n,)), ds.download(np.uint8, (n, sb)))
    finally:
        for b in (dg, db, dr, ds, do, dby, dmr):
            b.free()


SUBCH_IP = 64       # Subch.flags, with SUBCH_PACKET and without SUBCH_MOT: feed the entry's groups to the IP layer (Pipeline.ip)
IP_DELIVERED, IP_NOT_ACCEPTED, IP_TOO_LONG, IP_NOT_V4, IP_CHECKSUM, IP_NOT_UDP, IP_MALFORMED = range(7)   # dabgpu_ip_result.status
IP_STATE_DTYPE = np.dtype([("handled", "<i4"), ("crc_errors", "<i4")])                                    # dabgpu_ip_state
IP_RESULT_DTYPE = np.dtype([("offset", "<i4"), ("nbytes", "<i4"), ("status", "<i2"), ("quality", "<i2"),
                            ("ip_bytes", "<i4")])                                                         # dabgpu_ip_result
IP_RUN_DTYPE = np.dtype([("n_datagrams", "<i4"), ("n_bytes", "<i4"), ("counts", "<i4", (7,)), ("reserved", "<i4", (3,))])


def ip_arena_bytes(group_slots: int, arena_bytes: int) -> int:
    """DABGPU_IP_ARENA_FOR"""
    return arena_bytes + 16 * group_slots


def ip_groups(ctx: "Context", groups: np.ndarray, data: np.ndarray, run: np.ndarray,
              state: Optional[np.ndarray] = None, out_arena_bytes: Optional[int] = None):
    """ip_dataHandler::add_mscDatagroup per slot (dabgpu_ip_groups; ip-datahandler.cpp:40-127):
    groups [n_slots, group_slots] DATAGROUP_DTYPE, data [n_slots, arena] uint8 and run [n_slots]
    PACKET_RUN_DTYPE as Pipeline.packet() returns them for one stream; state [n_slots]
    IP_STATE_DTYPE carried from an earlier call (None: new ip_dataHandlers).  Returns (results
    [n_slots, group_slots] IP_RESULT_DTYPE -- the first run.n_groups of a row --, bytes [n_slots,
    out_arena] uint8, ip_run [n_slots] IP_RUN_DTYPE, state)."""
    groups = np.ascontiguousarray(groups, dtype=DATAGROUP_DTYPE)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    run = np.ascontiguousarray(run, dtype=PACKET_RUN_DTYPE)
    n, gs = groups.shape
    assert data.shape[0] == n and run.shape == (n,)
    st = np.zeros(n, IP_STATE_DTYPE) if state is None else np.ascontiguousarray(state, dtype=IP_STATE_DTYPE).reshape(n)
    oa = ip_arena_bytes(gs, data.shape[1]) if out_arena_bytes is None else int(out_arena_bytes)
    dg, db, dr, ds = ctx.put(groups.view(np.uint8)), ctx.put(data), ctx.put(run.view(np.uint8)), ctx.put(st.view(np.uint8))
    do = ctx.buf(max(16, n * gs * IP_RESULT_DTYPE.itemsize)).zero()
    dby, dir_ = ctx.buf(max(16, n * max(oa, 0))).zero(), ctx.buf(max(16, n * IP_RUN_DTYPE.itemsize)).zero()
    try:
        _chk(lib().dabgpu_ip_groups(ctx.h, ds.ptr, n, dg.ptr, gs, db.ptr, data.shape[1], dr.ptr, do.ptr, dby.ptr, oa, dir_.ptr),
             "dabgpu_ip_groups")
        ctx.sync()
        return (_records(do, IP_RESULT_DTYPE, (n, gs)), dby.download(np.uint8, (n, max(oa, 0))),
                _records(dir_, IP_RUN_DTYPE, (n,)), _records(ds, IP_STATE_DTYPE, (n,)))
    finally:
        for b in (dg, db, dr, ds, do, dby, dir_):
            b.free()


SUBCH_PAD = 32      # Subch.flags, with SUBCH_DABPLUS: feed the entry's good AUs to the PAD layer (Pipeline.pad)
PAD_LABEL_BYTES, PAD_LABEL_PIECES, PAD_LABEL_TRUNCATED = 256, 64, 1
PAD_LABEL_DTYPE = np.dtype([("cif", "<i4"), ("au", "<i4"), ("charset", "<i4"), ("nbytes", "<i4"), ("n_pieces", "<i4"),
                            ("flags", "<i4"), ("piece_len", "u1", (PAD_LABEL_PIECES,)),
                            ("text", "u1", (PAD_LABEL_BYTES,))])                                         # dabgpu_pad_label
PAD_RUN_DTYPE = np.dtype([("n_labels", "<i4"), ("n_groups", "<i4"), ("n_bytes", "<i4"), ("aus", "<i4"), ("pads", "<i4"),
                          ("unhandled", "<i4"), ("undefined", "<i4", (4,)), ("crc_failed", "<i4"),
                          ("guard_dropped", "<i4"), ("rejected_sf", "<i4"), ("reserved", "<i4", (3,))])  # dabgpu_pad_run


def pad_au_slots(n_frames: int) -> int:
    """DABGPU_PAD_AU_SLOTS"""
    return ((4 * n_frames + 4) // 5 + 1) * 6


def pad_arena_bytes(n_frames: int) -> int:
    """DABGPU_PAD_ARENA_BYTES"""
    return (8192 + pad_au_slots(n_frames) * 192 + 15) // 16 * 16


def pad_state_bytes() -> int:
    """dabgpu_pad_state_bytes: a padHandler's carried state (all zero: a new one)"""
    return int(lib().dabgpu_pad_state_bytes())


def pad_aus(ctx: "Context", aus: np.ndarray, lengths: np.ndarray, state: Optional[np.ndarray] = None,
            cif: Optional[np.ndarray] = None, label_slots: Optional[int] = None, group_slots: Optional[int] = None,
            arena_bytes: Optional[int] = None):
    """padHandler::processPAD per slot (dabgpu_pad_aus; pad-handler.cpp): aus [n_slots, n_aus,
    au_stride] uint8, lengths [n_slots, n_aus] int32 (the AU's aac_frame_length; negative: it
    failed its CRC), state [n_slots, pad_state_bytes()] bytes carried from an earlier call
    (None: new padHandlers), cif [n_slots, n_aus] int32 or None.  The slots default to four per
    AU and the arena to 8192 + 192 bytes per AU (at least pad_arena_bytes(0)).  Returns (labels [n_slots, label_slots]
    PAD_LABEL_DTYPE -- the first run.n_labels of a row --, groups [n_slots, group_slots]
    DATAGROUP_DTYPE, bytes [n_slots, arena] uint8, run [n_slots] PAD_RUN_DTYPE, state)."""
    aus = np.ascontiguousarray(aus, dtype=np.uint8)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    n, na, stride = aus.shape
    assert lengths.shape == (n, na)
    sb = pad_state_bytes()
    st = np.zeros((n, sb), np.uint8) if state is None else np.ascontiguousarray(state, dtype=np.uint8).reshape(n, sb)
    ls = 4 * na if label_slots is None else int(label_slots)
    gs = 4 * na if group_slots is None else int(group_slots)
    ar = max(pad_arena_bytes(0), (8192 + 192 * na + 15) // 16 * 16) if arena_bytes is None else int(arena_bytes)
    bufs = [ctx.put(aus) if aus.size else ctx.buf(16), ctx.put(lengths) if na and n else ctx.buf(16), ctx.put(st) if n else ctx.buf(16)]
    dc = None
    if cif is not None:
        cif = np.ascontiguousarray(cif, dtype=np.int32)
        assert cif.shape == (n, na)
        dc = ctx.put(cif) if cif.size else ctx.buf(16)
        bufs.append(dc)
    da, dl, ds = bufs[:3]
    dlab = ctx.buf(max(16, n * max(ls, 0) * PAD_LABEL_DTYPE.itemsize)).zero()
    dgr = ctx.buf(max(16, n * max(gs, 0) * DATAGROUP_DTYPE.itemsize)).zero()
    dby, drun = ctx.buf(max(16, n * max(ar, 0))).zero(), ctx.buf(max(16, n * PAD_RUN_DTYPE.itemsize)).zero()
    bufs += [dlab, dgr, dby, drun]
    try:
        _chk(lib().dabgpu_pad_aus(ctx.h, ds.ptr, n, da.ptr, stride, dl.ptr, na, dc.ptr if dc else None, dlab.ptr, ls,
                                  dgr.ptr, gs, dby.ptr, ar, drun.ptr), "dabgpu_pad_aus")
        ctx.sync()
        return (_records(dlab, PAD_LABEL_DTYPE, (n, ls)), _records(dgr, DATAGROUP_DTYPE, (n, gs)),
                dby.download(np.uint8, (n, ar)), _records(drun, PAD_RUN_DTYPE, (n,)), ds.download(np.uint8, (n, sb)))
    finally:
        for b in bufs:
            b.free()


# ---- FIC layer: the records of dabgpu_fib_parse (dabgpu.h) ----
_SUBCH_DTYPE = np.dtype([("startAddr", "<i2"), ("length", "<i2"), ("bitRate", "<i2"), ("protLevel", "<i2"),
                         ("uepFlag", "<i2"), ("flags", "<i2")])                                          # dabgpu_subch
FIC_TABLE_DTYPE = np.dtype([("n", "<i4"), ("reserved", "<i4", (3,)), ("sub", _SUBCH_DTYPE, (64,)),
                            ("ids", "u1", (64,))])                                                       # dabgpu_fic_table
FIC_DB_DTYPE = np.dtype([
    ("sub", np.dtype([("SubChId", "<i2"), ("StartAddr", "<i2"), ("Length", "<i2"), ("uepFlag", "<i2"), ("protLevel", "<i2"),
                      ("BitRate", "<i2"), ("FEC_scheme", "<i2"), ("inUse", "u1"), ("reserved", "u1")]), (64,)),
    ("components", np.dtype([("inUse", "u1"), ("TMid", "i1"), ("service", "<i2"), ("componentNr", "<i2"), ("ASCTy", "<i2"),
                             ("PS_flag", "<i2"), ("subchannelId", "<i2"), ("SCId", "<u2"), ("CAflag", "u1"), ("DGflag", "i1"),
                             ("DSCTy", "<i2"), ("packetAddress", "<i2")]), (64,)),
    ("services", np.dtype([("serviceId", "<i4"), ("inUse", "u1"), ("hasName", "u1"), ("hasLanguage", "u1"), ("charset", "u1"),
                           ("language", "<i2"), ("programType", "<i2"), ("data_suffix", "u1"), ("reserved", "u1", (3,)),
                           ("label", "u1", (16,))]), (64,)),
    ("EId", "<i4"), ("charset", "u1"), ("named", "u1"), ("reserved", "u1", (2,)), ("label", "u1", (16,)),
    ("reserved2", "u1", (8,)), ("table", FIC_TABLE_DTYPE)])                                              # dabgpu_fic_db
FIC_EVENT_DTYPE = np.dtype([("kind", "<i4"), ("fib", "<i4"), ("id", "<i4"), ("charset", "<i4"),
                            ("label", "u1", (16,))])                                                     # dabgpu_fic_event
FIC_RUN_DTYPE = np.dtype([("parsed", "<i4"), ("skipped", "<i4"), ("figs", "<i4", (8,)), ("n_events", "<i4"),
                          ("overrun", "<i4"), ("table_changed", "<i4"), ("reserved", "<i4", (3,))])      # dabgpu_fic_run
FIC_NAME_ENSEMBLE, FIC_ADD_SERVICE, FIC_EVENT_SLOTS = 1, 2, 65


def fic_db_bytes() -> int:
    """dabgpu_fic_db_bytes: a fib_processor's database as a record (all zero: a new one)"""
    return int(lib().dabgpu_fic_db_bytes())


def table_subch(table) -> list:
    """the Subch list of one FIC_TABLE_DTYPE record, as Pipeline.set_subch takes it"""
    return [Subch(*[int(x) for x in e]) for e in table["sub"][:int(table["n"])]]


def fib_parse(ctx: "Context", fibs: np.ndarray, ok: np.ndarray, db: Optional[np.ndarray] = None, want: int = 0,
              event_slots: int = FIC_EVENT_SLOTS, clear=None):
    """fib_processor::process_FIB per slot (dabgpu_fib_parse; fib-processor.cpp): fibs [n_slots,
    n_fibs, 32] uint8 (msb first, CRC bytes as delivered), ok [n_slots, n_fibs] uint8 (0: the FIB
    is skipped), db [n_slots] FIC_DB_DTYPE carried from an earlier call (None: new
    fib_processors), want the SUBCH_MP2 | PACKET | MOT | PAD bits the table may flag.  clear
    [n_slots] (optional): clearEnsemble for the slots it marks, before the parse
    (dabgpu_fic_clear).  Returns (db [n_slots] FIC_DB_DTYPE, events [n_slots, event_slots]
    FIC_EVENT_DTYPE -- the first min(run.n_events, event_slots) of a row --, table [n_slots]
    FIC_TABLE_DTYPE, run [n_slots] FIC_RUN_DTYPE)."""
    fibs = np.ascontiguousarray(fibs, dtype=np.uint8)
    n, nf = fibs.shape[:2]
    assert fibs.shape == (n, nf, 32)
    ok = np.ascontiguousarray(ok, dtype=np.uint8).reshape(n, nf)
    st = np.zeros(n, FIC_DB_DTYPE) if db is None else np.ascontiguousarray(db, dtype=FIC_DB_DTYPE).reshape(n)
    es = int(event_slots)
    ds = ctx.put(st.view(np.uint8)) if n else ctx.buf(16)
    df, dk = ctx.put(fibs) if fibs.size else ctx.buf(16), ctx.put(ok) if ok.size else ctx.buf(16)
    de = ctx.buf(max(16, n * max(es, 0) * FIC_EVENT_DTYPE.itemsize)).zero()
    dt, dr = ctx.buf(max(16, n * FIC_TABLE_DTYPE.itemsize)).zero(), ctx.buf(max(16, n * FIC_RUN_DTYPE.itemsize)).zero()
    try:
        if clear is not None:
            which = np.ascontiguousarray(clear, dtype=np.uint8).reshape(n)
            _chk(lib().dabgpu_fic_clear(ctx.h, ds.ptr, n, _p(which)), "dabgpu_fic_clear")
        _chk(lib().dabgpu_fib_parse(ctx.h, ds.ptr, n, df.ptr, 32 * nf, dk.ptr, nf, int(want), de.ptr, es, dt.ptr, dr.ptr),
             "dabgpu_fib_parse")
        ctx.sync()
        return (_records(ds, FIC_DB_DTYPE, (n,)), _records(de, FIC_EVENT_DTYPE, (n, max(es, 0))),
                _records(dt, FIC_TABLE_DTYPE, (n,)), _records(dr, FIC_RUN_DTYPE, (n,)))
    finally:
        for b in (ds, df, dk, de, dt, dr):
            b.free()


SUPERFRAME_DTYPE = np.dtype([("status", "i1"), ("num_aus", "i1"), ("n_corrected", "<i2"), ("au_start", "<i2", (7,)),
                             ("au_crc_ok", "u1"), ("reserved", "u1")])


class Superframe(C.Structure):
    """one CIF of one DAB+ subchannel through mp4Processor (mp4processor.cpp:107-292)"""
    _fields_ = [("status", C.c_int8), ("num_aus", C.c_int8), ("n_corrected", C.c_int16),
                ("au_start", C.c_int16 * 7), ("au_crc_ok", C.c_uint8), ("reserved", C.c_uint8)]


class Frame(C.Structure):
    _fields_ = [("iq_base", C.c_int64), ("n_samples", C.c_int64), ("window", C.c_int64), ("block0", C.c_int64),
                ("lp_window", C.c_int32), ("phase_a", C.c_int32), ("lp_data", C.c_int32),
                ("phase_b", C.c_int32), ("out_slot", C.c_int32), ("flags", C.c_int32)]


class PipeCaps(C.Structure):
    _fields_ = [("max_subch", C.c_int32), ("max_bitrate", C.c_int32), ("max_dabplus", C.c_int32),
                ("max_mp2", C.c_int32)]


class PipeCfg(C.Structure):
    _fields_ = [("n_streams", C.c_int32), ("n_frames", C.c_int32), ("n_subch", C.c_int32),
                ("threshold", C.c_int16), ("freq_sync_method", C.c_int16), ("subch", C.POINTER(Subch))]


class StreamState(C.Structure):
    _fields_ = [("next_pos", C.c_int64), ("local_phase", C.c_int32), ("coarse", C.c_int32),
                ("fine", C.c_int16), ("f2correction", C.c_int16), ("prev1", C.c_int16), ("prev2", C.c_int16),
                ("synced", C.c_int32), ("cif_count", C.c_int64), ("last_start_index", C.c_int32),
                ("resyncs", C.c_int32), ("acquisitions", C.c_int32), ("attempts", C.c_int32),
                ("no_signal", C.c_int32), ("frames_run", C.c_int32), ("acquiring", C.c_int32)]


class FrameInfo(C.Structure):
    """dabgpu_frame_info: per-frame observables of the last run (ofdm-processor.cpp:344-446,
    ofdm-decoder.cpp:93-97)"""
    _fields_ = [("window", C.c_int64), ("start_index", C.c_int32), ("coarse", C.c_int32), ("fine", C.c_int16),
                ("correction", C.c_int16), ("snr", C.c_int16), ("committed", C.c_int16)]


CTL_RESET, CTL_COARSE_ON, CTL_COARSE_OFF, CTL_SCAN_ON, CTL_SCAN_OFF, CTL_RESYNC = 1, 2, 3, 4, 5, 6
CTL_ACQ_ASYNC, CTL_ACQ_SYNC, CTL_INJECT_BOUNDS = 7, 8, 9
PACK_MSC, PACK_FIC = 1, 2          # dabgpu_pipe_set_packed mask


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libdabgpu.so (raises if it is missing: no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DabError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        l = C.CDLL(LIB_PATH)
        vp, i32, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
        sig = {
            "dabgpu_abi_version": ([], i32), "dabgpu_last_error": ([], C.c_char_p),
            "dabgpu_host_table": ([i32, vp, sz], i32),
            "dabgpu_subch_profile": ([vp, vp, vp, vp, vp, vp], i32),
            "dabgpu_device_count": ([], i32), "dabgpu_ctx_create": ([i32, C.POINTER(vp)], i32),
            "dabgpu_ctx_destroy": ([vp], i32), "dabgpu_sync": ([vp], i32),
            "dabgpu_alloc": ([vp, sz, C.POINTER(vp)], i32), "dabgpu_free": ([vp, vp], i32),
            "dabgpu_memcpy_h2d": ([vp, vp, vp, sz], i32), "dabgpu_memcpy_d2h": ([vp, vp, vp, sz], i32),
            "dabgpu_memset_d": ([vp, vp, i32, sz], i32),
            "dabgpu_memcpy_d2d": ([vp, vp, vp, sz], i32),
            "dabgpu_ofdm_symbol": ([vp, vp, i32, vp, vp], i32),
            "dabgpu_get_snr": ([vp, vp, vp], i32),
            "dabgpu_nco_eval": ([vp, i32, i32, vp], i32),
            "dabgpu_ofdm_demod_mix": ([vp, vp, i32, vp, i32, i32, C.c_int16, vp, vp, vp, vp], i32),
            "dabgpu_pipe_set_iq_format": ([vp, i32], i32),
            "dabgpu_pipe_acquire_wait": ([vp], i32),
            "dabgpu_pipe_set_display_token": ([vp, i32], i32),
            "dabgpu_iq_convert": ([vp, i32, vp, i64, vp], i32),
            "dabgpu_rate_convert": ([vp, i32, i32, vp, i64, i32, vp, vp, i64, vp, vp], i32),
            "dabgpu_event_record": ([vp, i32], i32),
            "dabgpu_kernel_errors": ([vp], i32),
            "dabgpu_event_elapsed": ([vp, i32, i32, C.POINTER(C.c_float)], i32),
            "dabgpu_prs_sync": ([vp, vp, vp, i32, C.c_int16, vp, vp, vp], i32),
            "dabgpu_block0": ([vp, vp, vp, i32, i32, vp, vp], i32),
            "dabgpu_ofdm_demod": ([vp, vp, vp, i32, vp, vp, vp], i32),
            "dabgpu_ofdm_sync_demod": ([vp, vp, vp, i32, C.c_int16, vp, vp, vp, vp, vp], i32),
            "dabgpu_viterbi": ([vp, vp, i32, i32, vp], i32),
            "dabgpu_fic_decode": ([vp, vp, i32, vp, vp], i32),
            "dabgpu_fic_decode_frames": ([vp, vp, vp, i32, vp, vp], i32),
            "dabgpu_msc_deconvolve": ([vp, vp, i64, vp, i32, vp, i64], i32),
            "dabgpu_rs_decode": ([vp, vp, i32, vp, vp], i32),
            "dabgpu_pipe_dabplus": ([vp, vp, C.c_int32, vp], i32),
            "dabgpu_mp2_decode": ([vp, vp, i64, i32, i32, vp, vp, vp], i32),
            "dabgpu_pipe_mp2": ([vp, vp, vp], i32),
            "dabgpu_audio_out": ([vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp], i32),
            "dabgpu_pipe_audio": ([vp, vp, vp, vp, vp], i32),
            "dabgpu_pipe_audio_caps": ([vp, i32], i32),
            "dabgpu_pipe_packet": ([vp, vp, vp, vp, vp], i32),
            "dabgpu_pipe_packet_caps": ([vp, i32, i32], i32),
            "dabgpu_mot_state_bytes": ([i32], sz),
            "dabgpu_mot_groups": ([vp, vp, i32, i32, vp, i32, vp, i64, vp, vp, vp, i64, vp], i32),
            "dabgpu_pad_state_bytes": ([], sz),
            "dabgpu_pad_aus": ([vp, vp, i32, vp, i64, vp, i32, vp, vp, i32, vp, i32, vp, i64, vp], i32),
            "dabgpu_fic_db_bytes": ([], sz),
            "dabgpu_fib_parse": ([vp, vp, i32, vp, i64, vp, i32, i32, vp, i32, vp, vp], i32),
            "dabgpu_fic_clear": ([vp, vp, i32, vp], i32),
            "dabgpu_pipe_fic_caps": ([vp, i32], i32),
            "dabgpu_pipe_fic": ([vp, vp, vp, i32, vp, vp, vp], i32),
            "dabgpu_pipe_fic_db": ([vp, i32, vp], i32),
            "dabgpu_pipe_fic_clear": ([vp, i32], i32),
            "dabgpu_pipe_mot": ([vp, vp, vp, vp], i32),
            "dabgpu_ip_groups": ([vp, vp, i32, vp, i32, vp, i64, vp, vp, vp, i64, vp], i32),
            "dabgpu_pipe_ip": ([vp, vp, vp, vp], i32),
            "dabgpu_pipe_ip_state": ([vp, i32, vp], i32),
            "dabgpu_pipe_pad": ([vp, vp, i32, vp, vp, vp, vp, vp], i32),
            "dabgpu_pipe_pad_caps": ([vp, i32], i32),
            "dabgpu_pipe_mot_caps": ([vp, i32, i32], i32),
            "dabgpu_pipe_sync": ([vp], i32),
            "dabgpu_pipe_create": ([vp, vp, C.POINTER(vp)], i32), "dabgpu_pipe_destroy": ([vp], i32),
            "dabgpu_pipe_acquire": ([vp, vp, i64, vp, vp], i32),
            "dabgpu_pipe_run": ([vp, vp, i64, vp, vp, vp, vp, C.c_int32, vp], i32),
            "dabgpu_pipe_state": ([vp, i32, vp], i32),
            "dabgpu_pipe_frame_info": ([vp, vp], i32),
            "dabgpu_pipe_control": ([vp, i32, i32], i32),
            "dabgpu_pipe_softbits": ([vp, C.POINTER(vp), C.POINTER(C.c_int32)], i32),
            "dabgpu_pipe_set_dabplus_compact": ([vp, i32], i32),
            "dabgpu_pipe_frame_slot": ([vp, i32, C.POINTER(C.c_int32)], i32),
            "dabgpu_pipe_frames": ([vp, vp, vp], i32),
            "dabgpu_pipe_set_display": ([vp, i32], i32),
            "dabgpu_pipe_set_packed": ([vp, i32], i32),
            "dabgpu_pipe_fetch": ([vp, vp, vp, sz], i32),
            "dabgpu_host_alloc": ([vp, sz, C.POINTER(vp)], i32),
            "dabgpu_host_free": ([vp, vp], i32),
            "dabgpu_pipe_iq_display": ([vp, i32, i32, vp], i32),
            "dabgpu_pipe_set_profiling": ([vp, i32], i32),
            "dabgpu_pipe_timing": ([vp, vp, vp], i32),
            "dabgpu_pipe_create_caps": ([vp, vp, vp, C.POINTER(vp)], i32),
            "dabgpu_pipe_set_subch": ([vp, i32, vp, C.c_int32], i32),
            "dabgpu_pipe_get_subch": ([vp, i32, vp, C.POINTER(C.c_int32), vp], i32),
            "dabgpu_pipe_msc_entry_valid": ([vp, vp], i32),
        }
        for name, (args, res) in sig.items():
            try:
                f = getattr(l, name)
            except AttributeError:
                if "DABGPU_LIB" in os.environ:           # an older A/B build (tools/): calls to it raise
                    continue
                raise
            f.argtypes, f.restype = args, res
        _lib = l
    return _lib


def _chk(rc: int, what: str) -> None:
    if rc != 0:
        e = DabError(f"{what} failed ({rc}): {lib().dabgpu_last_error().decode()}")
        e.code = rc                                          # the DABGPU_E_* code
        raise e


def _p(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


IQ_F32, IQ_U8, IQ_S16 = 0, 1, 2   # sample formats (dabgpu_iq_convert, dabgpu_pipe_set_iq_format)
IQ_S12 = 3                        # int16 pairs holding the Airspy's 12-bit samples, x / 2048 (dabgpu_rate_convert only)
TABLE_PRS, TABLE_MAPPER, TABLE_REFARG, TABLE_OSC, TABLE_NCO = 1, 2, 3, 4, 5


def host_table(which: int) -> np.ndarray:
    """the product's host-built tables (dabgpu_host_table; no device needed)"""
    shape, dt = {TABLE_PRS: ((2048, 2), np.float32), TABLE_MAPPER: (1536, np.int16),
                 TABLE_REFARG: (18, np.float32), TABLE_OSC: ((2048000, 2), np.float32),
                 TABLE_NCO: ((384, 2), np.float64), TABLE_AUDIO_FIR: ((3, 5), np.float32)}[which]
    out = np.zeros(shape, dt)
    _chk(lib().dabgpu_host_table(which, _p(out), out.nbytes), "dabgpu_host_table")
    return out


def subch_profile(sub: "Subch"):
    """(nbits, fragment size, [(L_i, PI_i)...], fallback) of the decoder's depuncturing
    profile for a subchannel (dabgpu_subch_profile)"""
    nb, fr, ns = C.c_int32(), C.c_int32(), C.c_int32()
    L, PI = np.zeros(4, np.int32), np.zeros(4, np.int32)
    rc = lib().dabgpu_subch_profile(C.byref(sub), C.byref(nb), C.byref(fr), C.byref(ns), _p(L), _p(PI))
    if rc < 0:
        _chk(rc, "dabgpu_subch_profile")
    return nb.value, fr.value, [(int(L[k]), int(PI[k])) for k in range(ns.value)], rc == 1


def read_raw(path: str) -> np.ndarray:
    """.raw recording (rawfiles.cpp): interleaved unsigned 8-bit I/Q, no header.
    Returns the bytes memory-mapped (an odd trailing byte is dropped)."""
    a = np.memmap(path, dtype=np.uint8, mode="r")
    return a[: a.size & ~1]


def read_sdr(path: str) -> np.ndarray:
    """.sdr recording (wavfiles.cpp:56-69): a WAV file with 2 channels (I, Q) of
    PCM16 at 2048000 samples/s.  Returns the interleaved int16 samples
    memory-mapped; raises ValueError for any other WAV layout, as the reference
    refuses it ("This is not a recorded dab file")."""
    import struct
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt = None
        off = 12
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise ValueError(f"{path}: no data chunk")
            cid, n = ck[:4], struct.unpack("<I", ck[4:])[0]
            off += 8
            if cid == b"fmt ":
                b = f.read(n)
                tag, ch, rate, _, _, bits = struct.unpack("<HHIIHH", b[:16])
                if tag == 0xFFFE and n >= 26:              # WAVE_FORMAT_EXTENSIBLE: subformat GUID
                    tag = struct.unpack("<H", b[24:26])[0]
                fmt = (tag, ch, rate, bits)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: data before fmt chunk")
                if fmt != (1, 2, 2048000, 16):
                    raise ValueError(f"{path}: not a recorded DAB file (format/channels/rate/bits {fmt}); "
                                     "need PCM16, 2 channels, 2048000 Hz")
                size = os.path.getsize(path)
                n = min(n, size - off) & ~3
                return np.memmap(path, dtype="<i2", mode="r", offset=off, shape=(n // 2,))
            else:
                f.seek(n + (n & 1), 1)
            off += n + (n & 1)


def write_sdr(path: str, iq_s16: np.ndarray) -> None:
    """write interleaved int16 I/Q as an .sdr WAV (2 channels, PCM16, 2048000 Hz):
    the recording format of gui.cpp:880-883"""
    import wave
    with wave.open(path, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(2048000)
        w.writeframes(np.ascontiguousarray(iq_s16, dtype="<i2").tobytes())


class DevBuf:
    """HBM buffer owned by a Context."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _chk(lib().dabgpu_alloc(ctx.h, max(self.nbytes, 16), C.byref(p)), "dabgpu_alloc")
        self.ptr = p

    def upload(self, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        _chk(lib().dabgpu_memcpy_h2d(self.ctx.h, self.ptr, _p(a), a.nbytes), "h2d")
        return self

    def upload_at(self, a: np.ndarray, offset: int) -> "DevBuf":
        """copy `a` to byte `offset` of the buffer"""
        a = np.ascontiguousarray(a)
        assert offset >= 0 and offset + a.nbytes <= self.nbytes
        _chk(lib().dabgpu_memcpy_h2d(self.ctx.h, C.c_void_p(self.ptr.value + offset), _p(a), a.nbytes), "h2d")
        return self

    def download(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _chk(lib().dabgpu_memcpy_d2h(self.ctx.h, _p(out), self.ptr, out.nbytes), "d2h")
        return out

    def zero(self) -> "DevBuf":
        return self.fill(0)

    def fill(self, value: int) -> "DevBuf":
        """every byte := value (on the context's stream, ahead of the operators that follow)"""
        _chk(lib().dabgpu_memset_d(self.ctx.h, self.ptr, int(value) & 0xFF, self.nbytes), "memset")
        return self

    def free(self) -> None:
        if self.ptr:
            lib().dabgpu_free(self.ctx.h, self.ptr)
            self.ptr = None


class HostBuf:
    """page-locked host memory (dabgpu_host_alloc): the target of Pipeline.fetch"""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _chk(lib().dabgpu_host_alloc(ctx.h, max(self.nbytes, 16), C.byref(p)), "dabgpu_host_alloc")
        self.ptr = p

    def view(self, dtype, shape, offset: int = 0) -> np.ndarray:
        """a numpy view of the memory (valid until free)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert offset + n <= self.nbytes
        raw = (C.c_uint8 * n).from_address(self.ptr.value + offset)
        return np.frombuffer(raw, dtype=dtype).reshape(shape)

    def free(self) -> None:
        if self.ptr:
            lib().dabgpu_host_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """One HIP device + stream (dabgpu_ctx)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _chk(lib().dabgpu_ctx_create(device, C.byref(h)), "dabgpu_ctx_create")
        self.h = h

    def buf(self, nbytes: int) -> DevBuf:
        return DevBuf(self, nbytes)

    def put(self, a: np.ndarray) -> DevBuf:
        a = np.ascontiguousarray(a)
        return DevBuf(self, a.nbytes).upload(a)

    def sync(self) -> None:
        _chk(lib().dabgpu_sync(self.h), "sync")

    def iq_convert(self, fmt: int, src: "DevBuf", n_pairs: int, dst: "DevBuf", src_off: int = 0,
                   dst_off: int = 0) -> None:
        """dabgpu_iq_convert: recorded samples (IQ_U8 / IQ_S16) in src -> cf32 in dst"""
        _chk(lib().dabgpu_iq_convert(self.h, fmt, C.c_void_p(src.ptr.value + src_off), n_pairs,
                                     C.c_void_p(dst.ptr.value + dst_off)), "dabgpu_iq_convert")

    def rate_convert(self, rate: int, fmt: int, src: "DevBuf", src_stride: int, n_in, dst: "DevBuf", dst_stride: int,
                     src_off: int = 0, dst_off: int = 0):
        """dabgpu_rate_convert: streams sampled at rate Hz (n_in[s] samples of format fmt at sample
        src_stride * s of src) -> 2.048 MHz cf32 at sample dst_stride * s of dst, as airspyHandler
        converts them.  Asynchronous (sync() to wait).  Returns (n_out, n_used), int64 per stream:
        sample n_used[s] of a stream is the first sample of its next call."""
        n_in = np.ascontiguousarray(n_in, np.int64)
        n_out, n_used = np.zeros(len(n_in), np.int64), np.zeros(len(n_in), np.int64)
        _chk(lib().dabgpu_rate_convert(self.h, int(rate), int(fmt), C.c_void_p(src.ptr.value + src_off), int(src_stride),
                                       len(n_in), _p(n_in), C.c_void_p(dst.ptr.value + dst_off), int(dst_stride),
                                       _p(n_out), _p(n_used)), "dabgpu_rate_convert")
        return n_out, n_used

    def load_iq_file(self, path: str, max_pairs: Optional[int] = None, chunk_pairs: int = 1 << 25):
        """Read a .raw (u8) or .sdr (WAV PCM16) recording into HBM as interleaved cf32,
        converting on the GPU; streamed in chunks (host memory stays at one chunk).
        Returns (DevBuf, n_pairs)."""
        if path.endswith(".raw"):
            src, fmt, w = read_raw(path), IQ_U8, 1
        else:
            src, fmt, w = read_sdr(path), IQ_S16, 2
        n = src.size // 2
        if max_pairs is not None:
            n = min(n, int(max_pairs))
        dst = self.buf(max(8 * n, 16))
        stage = self.buf(2 * w * min(n, chunk_pairs) + 16)
        try:
            for p0 in range(0, n, chunk_pairs):
                m = min(chunk_pairs, n - p0)
                stage.upload(np.ascontiguousarray(src[2 * p0: 2 * (p0 + m)]))
                self.iq_convert(fmt, stage, m, dst, dst_off=8 * p0)
                self.sync()
        finally:
            stage.free()
        return dst, n

    def load_recording(self, path: str, max_pairs: Optional[int] = None, chunk_pairs: int = 1 << 25):
        """Read a .raw (u8) or .sdr (WAV PCM16) recording into HBM as the file holds it
        (2 or 4 bytes per I/Q pair, a quarter / half of cf32): the pipeline converts it in
        its kernels' loads (Pipeline.set_iq_format(fmt), exactly as the reference's readers
        do, rawfiles.cpp:115-117 / wavfiles.cpp:172).  Streamed in chunks from the
        memory-mapped file.  Returns (DevBuf, n_pairs, fmt)."""
        if path.endswith(".raw"):
            src, fmt, w = read_raw(path), IQ_U8, 1
        else:
            src, fmt, w = read_sdr(path), IQ_S16, 2
        n = src.size // 2
        if max_pairs is not None:
            n = min(n, int(max_pairs))
        dst = self.buf(max(2 * w * n, 16))
        for p0 in range(0, n, chunk_pairs):
            m = min(chunk_pairs, n - p0)
            dst.upload_at(np.ascontiguousarray(src[2 * p0: 2 * (p0 + m)]), 2 * w * p0)
        return dst, n, fmt

    def check(self) -> None:
        """raise if a kernel refused out-of-bounds work since the last check"""
        _chk(lib().dabgpu_kernel_errors(self.h), "kernel bounds check")

    def close(self) -> None:
        if self.h:
            lib().dabgpu_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- operators mirroring the reference interfaces -------------------------
    @staticmethod
    def _out_at(out: Optional[DevBuf], out_offset: int, extent: int) -> C.c_void_p:
        """the device address of byte out_offset of a caller's output buffer, of which the
        operator may write [out_offset, out_offset + extent)"""
        if out_offset < 0 or out_offset + extent > out.nbytes:
            raise DabError(f"output of {extent} bytes at offset {out_offset} does not fit the {out.nbytes}-byte buffer")
        return C.c_void_p(out.ptr.value + out_offset)

    def viterbi(self, soft: np.ndarray, nbits: int, out: Optional[DevBuf] = None, out_offset: int = 0) -> np.ndarray:
        """viterbi::deconvolve (viterbi.cpp:225-242) for each row of soft [n, 4*(nbits+6)].
        out: the caller's buffer, which receives the rows from byte out_offset on (and stays
        the caller's: download all of it to see what else was written); else a fresh one."""
        soft = np.ascontiguousarray(soft, dtype=np.int16).reshape(-1, 4 * (nbits + 6))
        n = soft.shape[0]
        din = self.put(soft) if n else self.buf(16)
        dout = self.buf(n * nbits) if out is None else None
        try:
            po = dout.ptr if out is None else self._out_at(out, out_offset, n * nbits)
            _chk(lib().dabgpu_viterbi(self.h, din.ptr, n, nbits, po), "dabgpu_viterbi")
            if n == 0:
                self.sync()
                r = np.zeros((0, nbits), np.uint8)
            elif out is None:
                r = dout.download(np.uint8, (n, nbits))
            else:
                r = out.download(np.uint8, out.nbytes)[out_offset:out_offset + n * nbits].reshape(n, nbits)
            self.check()
            return r
        finally:
            din.free()
            if dout is not None:
                dout.free()

    def fic_process(self, blocks: np.ndarray, out: Optional[DevBuf] = None, out_offset: int = 0):
        """ficHandler::process_ficInput (fic-handler.cpp:241-321) for [n, 2304] soft bits.
        Returns (bits [n,768] after energy dispersal and the CRC check's inversion, crc_ok [n,3]).
        out: the caller's buffer for the bits, from byte out_offset on (a multiple of 4: the
        CRC check reads them as words); else a fresh one."""
        blocks = np.ascontiguousarray(blocks, dtype=np.int16).reshape(-1, 2304)
        n = blocks.shape[0]
        if out is not None and out_offset % 4:
            raise DabError("fic_process: out_offset must be a multiple of 4")
        din, dc = self.put(blocks), self.buf(n * 3)
        db = self.buf(n * 768) if out is None else None
        try:
            pb = db.ptr if out is None else self._out_at(out, out_offset, n * 768)
            _chk(lib().dabgpu_fic_decode(self.h, din.ptr, n, pb, dc.ptr), "dabgpu_fic_decode")
            if out is None:
                bits = db.download(np.uint8, (n, 768))
            else:
                bits = out.download(np.uint8, out.nbytes)[out_offset:out_offset + n * 768].reshape(n, 768)
            return bits, dc.download(np.uint8, (n, 3))
        finally:
            din.free(); dc.free()
            if db is not None:
                db.free()

    def fic_decode_frames(self, soft: DevBuf, slots: Sequence[int]):
        """dabgpu_fic_decode_frames: the four FIC blocks of each frame slots[i] of a demod
        soft-bit buffer (int16 [slot][75][3072] on the device; the first 9216 values of a slot
        are read).  Returns (bits [n, 4, 768], crc_ok [n, 12]) as fic_process does per block."""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        n = len(sl)
        if n and (sl.min() < 0 or 2 * (int(sl.max()) + 1) * NSYM * SYMBITS > soft.nbytes):
            raise DabError("fic_decode_frames: a slot outside the soft-bit buffer")
        db, dc = self.buf(max(1, n * 4 * 768)), self.buf(max(1, n * 12))
        try:
            _chk(lib().dabgpu_fic_decode_frames(self.h, soft.ptr, _p(sl), n, db.ptr, dc.ptr), "dabgpu_fic_decode_frames")
            if n == 0:
                return np.zeros((0, 4, 768), np.uint8), np.zeros((0, 12), np.uint8)
            return db.download(np.uint8, (n, 4, 768)), dc.download(np.uint8, (n, 12))
        finally:
            db.free(); dc.free()

    def msc_deconvolve(self, frags: np.ndarray, subch: Sequence[Subch], out: Optional[DevBuf] = None,
                       out_offset: int = 0, out_stride: Optional[int] = None) -> list:
        """uep_/eep_deconvolve::deconvolve + energy dispersal (deconvolve.cpp:172,325;
        dab-concurrent.cpp:183-190): one already de-interleaved fragment per row.
        out_stride: bytes from one codeword's bits to the next's (default: the longest
        codeword's 24*bitRate); out: the caller's buffer, row i at byte out_offset +
        i*out_stride (it stays the caller's); else a fresh one."""
        frags = np.ascontiguousarray(frags, dtype=np.int16)
        n, stride = frags.shape
        arr = (Subch * n)(*subch)
        nb = [24 * s.bitRate for s in subch]
        ostride = max(nb) if out_stride is None else int(out_stride)
        extent = max(i * ostride + max(nb[i], 0) for i in range(n))     # the last byte any row may take
        din = self.put(frags)
        dout = self.buf(max(extent, n * max(nb))) if out is None else None
        try:
            po = dout.ptr if out is None else self._out_at(out, out_offset, extent)
            _chk(lib().dabgpu_msc_deconvolve(self.h, din.ptr, stride, C.cast(arr, C.c_void_p), n, po, ostride),
                 "dabgpu_msc_deconvolve")
            if out is None:
                flat = dout.download(np.uint8, dout.nbytes)
            else:
                flat = out.download(np.uint8, out.nbytes)[out_offset:]
            return [flat[i * ostride:i * ostride + nb[i]] for i in range(n)]
        finally:
            din.free()
            if dout is not None:
                dout.free()

    def rs_decode(self, cw: np.ndarray):
        """reedSolomon::dec(rsIn, rsOut, 135) per row (reed-solomon.cpp:129-141):
        [n, 120] bytes -> ([n, 110] corrected bytes, [n] symbols corrected or -1)."""
        cw = np.ascontiguousarray(cw, dtype=np.uint8)
        n = cw.shape[0]
        din, dout, dr = self.put(cw), self.buf(max(1, 110 * n)), self.buf(max(2, 2 * n))
        try:
            _chk(lib().dabgpu_rs_decode(self.h, din.ptr, n, dout.ptr, dr.ptr), "dabgpu_rs_decode")
            return dout.download(np.uint8, (n, 110)), dr.download(np.int16, n)
        finally:
            din.free(); dout.free(); dr.free()

    def mp2_decode(self, frames: np.ndarray, chain_len: int, state: Optional[np.ndarray] = None):
        """mp2Processor::mp2decodeFrame per row (mp2processor.cpp:365-568): frames
        [n_chains * chain_len, stride] bytes, chain_len consecutive rows to each decoder in
        order; state [n_chains, MP2_STATE_BYTES] bytes carried from an earlier call (None:
        new decoders).  Returns (pcm [n_chains, chain_len, 1152, 2] int16 -- zeros where the
        frame was rejected --, ret [n_chains, chain_len] int32, state)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, stride = frames.shape
        if chain_len <= 0 or n % chain_len:
            raise DabError("mp2_decode: rows are not a multiple of chain_len")
        nc = n // chain_len
        st = np.zeros((nc, MP2_STATE_BYTES), np.uint8) if state is None else \
            np.ascontiguousarray(state, dtype=np.uint8).reshape(nc, MP2_STATE_BYTES)
        din, ds = self.put(frames), self.put(st)
        dp, dr = self.buf(max(1, n * 1152 * 4)).zero(), self.buf(max(4, 4 * n))
        try:
            _chk(lib().dabgpu_mp2_decode(self.h, din.ptr, stride, nc, chain_len, ds.ptr, dp.ptr, dr.ptr),
                 "dabgpu_mp2_decode")
            self.sync()
            return (dp.download(np.int16, (nc, chain_len, 1152, 2)), dr.download(np.int32, (nc, chain_len)),
                    ds.download(np.uint8, (nc, MP2_STATE_BYTES)))
        finally:
            din.free(); ds.free(); dp.free(); dr.free()

    def audio_out(self, pcm: np.ndarray, rates, amounts, state: Optional[np.ndarray] = None, fill: Optional[float] = None):
        """audioSink::audioOut per call (audiosink.cpp:235-360): pcm [n_chains, chain_len, max_amount, 2]
        int16, rates and amounts [n_chains, chain_len] (rate 0: no call), chain_len consecutive calls
        to each sink in order; state [n_chains, AUDIO_STATE_BYTES] bytes carried from an earlier call
        (None: new sinks).  Returns (samples [n_chains, chain_len, 3 * max_amount, 2] float32 -- the
        first n_out pairs of a row are the call's, the rest keeps `fill` (None: zeros) --, n_out
        [n_chains, chain_len] int32, state)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        nc, cl, ma, two = pcm.shape
        if two != 2:
            raise DabError("audio_out: pcm is [n_chains, chain_len, max_amount, 2]")
        ra = np.ascontiguousarray(rates, dtype=np.int32).reshape(nc, cl)
        am = np.ascontiguousarray(amounts, dtype=np.int32).reshape(nc, cl)
        st = np.zeros((nc, AUDIO_STATE_BYTES), np.uint8) if state is None else \
            np.ascontiguousarray(state, dtype=np.uint8).reshape(nc, AUDIO_STATE_BYTES)
        n = nc * cl
        din, ds = self.put(pcm if pcm.size else np.zeros(2, np.int16)), self.put(st if st.size else np.zeros(32, np.uint8))
        out = np.zeros((nc, cl, 3 * ma, 2), np.float32) if fill is None else np.full((nc, cl, 3 * ma, 2), fill, np.float32)
        do, dn = self.put(out if out.size else np.zeros(2, np.float32)), self.buf(max(4, 4 * n))
        try:
            _chk(lib().dabgpu_audio_out(self.h, din.ptr, ma, nc, cl, ma, _p(ra), _p(am), ds.ptr, do.ptr, dn.ptr),
                 "dabgpu_audio_out")
            self.sync()
            return (do.download(np.float32, (nc, cl, 3 * ma, 2)), dn.download(np.int32, (nc, cl)),
                    ds.download(np.uint8, (nc, AUDIO_STATE_BYTES)))
        finally:
            din.free(); ds.free(); do.free(); dn.free()

    def prs_sync(self, iq: DevBuf, frames: Sequence[Frame], level: int = 3):
        """phaseReference::findIndex (phasereference.cpp:60-88) per frame window."""
        n = len(frames)
        fa = (Frame * n)(*frames)
        dfr = DevBuf(self, C.sizeof(fa)).upload(np.frombuffer(fa, dtype=np.uint8))
        dsi, dmx, dsm = self.buf(4 * n), self.buf(4 * n), self.buf(4 * n)
        try:
            _chk(lib().dabgpu_prs_sync(self.h, iq.ptr, dfr.ptr, n, level, dsi.ptr, dmx.ptr, dsm.ptr), "prs_sync")
            r = (dsi.download(np.int32, n), dmx.download(np.float32, n), dsm.download(np.float32, n))
            self.check()
            return r
        finally:
            for b in (dfr, dsi, dmx, dsm):
                b.free()

    def block0(self, iq: DevBuf, frames: Sequence[Frame], method: int = 1, with_snr: bool = False):
        """ofdmDecoder::processBlock_0 (ofdm-decoder.cpp:85-162): coarse offset of
        freqSyncMethod `method` (frames with flags & 1), and get_snr when with_snr."""
        n = len(frames)
        fa = (Frame * n)(*frames)
        dfr = DevBuf(self, C.sizeof(fa)).upload(np.frombuffer(fa, dtype=np.uint8))
        dc, ds = self.buf(2 * n), self.buf(2 * n)
        try:
            _chk(lib().dabgpu_block0(self.h, iq.ptr, dfr.ptr, n, method, dc.ptr, ds.ptr), "block0")
            r = dc.download(np.int16, n)
            snr = ds.download(np.int16, n)
            self.check()
            return (r, snr) if with_snr else r
        finally:
            dfr.free(); dc.free(); ds.free()

    def demod(self, iq: DevBuf, frames: Sequence[Frame], with_float: bool = False):
        """ofdmDecoder::processToken for symbols 1..75 (ofdm-decoder.cpp:167-190).
        Frame i must have out_slot == i.  Returns (ibits [n,75,3072], softf or None, freqcorr [n] complex)."""
        n = len(frames)
        fa = (Frame * n)(*frames)
        dfr = DevBuf(self, C.sizeof(fa)).upload(np.frombuffer(fa, dtype=np.uint8))
        ds = self.buf(2 * n * NSYM * SYMBITS)
        df = self.buf(4 * n * NSYM * SYMBITS) if with_float else None
        dfc = self.buf(8 * n)
        try:
            _chk(lib().dabgpu_ofdm_demod(self.h, iq.ptr, dfr.ptr, n, ds.ptr, df.ptr if df else None, dfc.ptr),
                 "ofdm_demod")
            soft = ds.download(np.int16, (n, NSYM, SYMBITS))
            softf = df.download(np.float32, (n, NSYM, SYMBITS)) if df else None
            fc = dfc.download(np.float32, (n, 2))
            self.check()
            return soft, softf, fc[:, 0] + 1j * fc[:, 1]
        finally:
            for b in (dfr, ds, df, dfc):
                if b is not None:
                    b.free()


    def demod_mix(self, iq: DevBuf, frames: Sequence[Frame], chunks: int = 1, fmt: int = None, level: int = 3,
                  with_spec: bool = False):
        """dabgpu_ofdm_demod_mix: the fused demod's NCO-mixed FFT input of every data
        symbol, float32 [n, 75, 2048, 2] (samples [T_g, T_s) of symbol l after getSamples'
        NCO), and the soft bits; `chunks` workgroups per frame.
        fmt None: the operator form (cf32 in, frames give block0; int16 soft bits [n, 75, 3072]).
        fmt IQ_F32 / IQ_S16 / IQ_U8: the pipeline's instantiation (findIndex on each frame's
        window, samples read in that format, RING8 soft bytes [n, 75, 3072] u8); the start
        indices are returned too.  Returns (mix, soft) -- (mix, soft, start_index) with fmt --
        and the FFT output [n, 75, 2048] complex64 (natural bins) last when with_spec."""
        n = len(frames)
        fa = (Frame * n)(*frames)
        dfr = DevBuf(self, C.sizeof(fa)).upload(np.frombuffer(fa, dtype=np.uint8))
        dm = self.buf(8 * n * NSYM * 2048)
        dp = self.buf(8 * n * NSYM * 2048)
        sync = fmt is not None
        ds = self.buf((1 if sync else 2) * n * NSYM * SYMBITS)
        dsi = self.buf(4 * n) if sync else None
        try:
            _chk(lib().dabgpu_ofdm_demod_mix(self.h, iq.ptr, IQ_F32 if fmt is None else fmt, dfr.ptr, n, chunks, level,
                                             dsi.ptr if sync else None, dm.ptr, dp.ptr, ds.ptr), "ofdm_demod_mix")
            mix = dm.download(np.float32, (n, NSYM, 2048, 2))
            soft = ds.download(np.uint8 if sync else np.int16, (n, NSYM, SYMBITS))
            out = (mix, soft) + ((dsi.download(np.int32, n),) if sync else ())
            if with_spec:
                sp = dp.download(np.float32, (n, NSYM, 2048, 2))
                out += (sp[..., 0] + 1j * sp[..., 1],)
            self.check()
            return out
        finally:
            for b in (dfr, dm, dp, ds, dsi):
                if b is not None:
                    b.free()

    def ofdm_symbol(self, samples: np.ndarray, kind: int = 0, spectrum: Optional[np.ndarray] = None):
        """dabgpu_ofdm_symbol (ofdmDecoder::processBlock_0 / processToken one symbol at a
        time): kind 0 = FFT of T_u samples (complex64 [2048]) -> the spectrum in natural bin
        order; kind 1 = a data symbol (T_s samples) against `spectrum` -> (ibits [3072],
        the new spectrum)."""
        x = np.ascontiguousarray(samples, dtype=np.complex64).view(np.float32)
        ds, dsp = self.put(x), self.buf(8 * 2048)
        db = self.buf(2 * SYMBITS) if kind else None
        try:
            if spectrum is not None:
                dsp.upload(np.ascontiguousarray(spectrum, dtype=np.complex64).view(np.float32))
            _chk(lib().dabgpu_ofdm_symbol(self.h, ds.ptr, kind, dsp.ptr, db.ptr if db else None), "ofdm_symbol")
            sp = dsp.download(np.float32, (2048, 2))
            self.check()
            spec = sp[:, 0] + 1j * sp[:, 1]
            return (db.download(np.int16, SYMBITS), spec) if kind else spec
        finally:
            for b in (ds, dsp, db):
                if b is not None:
                    b.free()

    def nco_eval(self, first: int = 0, n: int = 2048000) -> np.ndarray:
        """oscillatorTable[first:first+n] as the front-end kernels compute it
        (dabgpu_nco_eval): float32 [n, 2]"""
        d = self.buf(8 * n)
        try:
            _chk(lib().dabgpu_nco_eval(self.h, first, n, d.ptr), "nco_eval")
            out = d.download(np.float32, (n, 2))
            self.check()
            return out
        finally:
            d.free()

    def sync_demod(self, iq: DevBuf, frames: Sequence[Frame], level: int = 3, with_float: bool = False):
        """findIndex + get_snr + processToken x 75 in one launch (dabgpu_ofdm_sync_demod).
        Frame i must have out_slot == i.  Returns (start_index [n], snr [n], ibits [n,75,3072],
        softf or None, freqcorr [n] complex)."""
        n = len(frames)
        fa = (Frame * n)(*frames)
        dfr = DevBuf(self, C.sizeof(fa)).upload(np.frombuffer(fa, dtype=np.uint8))
        dsi, dsn = self.buf(4 * n), self.buf(2 * n)
        ds = self.buf(2 * n * NSYM * SYMBITS)
        df = self.buf(4 * n * NSYM * SYMBITS) if with_float else None
        dfc = self.buf(8 * n)
        try:
            _chk(lib().dabgpu_ofdm_sync_demod(self.h, iq.ptr, dfr.ptr, n, level, dsi.ptr, dsn.ptr, ds.ptr,
                                              df.ptr if df else None, dfc.ptr), "ofdm_sync_demod")
            si = dsi.download(np.int32, n)
            snr = dsn.download(np.int16, n)
            soft = ds.download(np.int16, (n, NSYM, SYMBITS))
            softf = df.download(np.float32, (n, NSYM, SYMBITS)) if df else None
            fc = dfc.download(np.float32, (n, 2))
            self.check()
            return si, snr, soft, softf, fc[:, 0] + 1j * fc[:, 1]
        finally:
            for b in (dfr, dsi, dsn, ds, df, dfc):
                if b is not None:
                    b.free()


class Pipeline:
    """ofdmProcessor::run + ficHandler + mscHandler for n_streams ensembles
    (ofdm-processor.cpp:247-474, fic-handler.cpp:192-321, msc-handler.cpp:125-193,
    dab-concurrent.cpp:144-193), n_frames frames per run() call.

    subch is every stream's initial table.  With any of max_subch / max_bitrate / max_dabplus
    (dabgpu_pipe_create_caps; one left None is taken from subch) the pipeline is sized by
    those caps and set_subch(stream, subs) may give each stream its own table between runs:
    run() then returns msc [S, 4F, max_subch, stride] (entry k of a stream in row k) and
    dabplus() records and bytes with max_dabplus slots."""

    def __init__(self, ctx: Context, n_streams: int, n_frames: int, subch: Sequence[Subch],
                 threshold: int = 3, freq_sync_method: int = 1, max_subch: Optional[int] = None,
                 max_bitrate: Optional[int] = None, max_dabplus: Optional[int] = None,
                 max_mp2: Optional[int] = None, max_packet: Optional[int] = None,
                 max_group_bytes: Optional[int] = None, max_mot: Optional[int] = None,
                 max_body_bytes: Optional[int] = None):
        self.ctx, self.S, self.F, self.subch = ctx, n_streams, n_frames, list(subch)
        self._arr = (Subch * max(1, len(self.subch)))(*self.subch)
        cfg = PipeCfg(n_streams, n_frames, len(self.subch), threshold, freq_sync_method,
                      C.cast(self._arr, C.POINTER(Subch)))
        h = C.c_void_p()
        own = (len(self.subch), max([s.bitRate for s in self.subch] + [0]),
               sum(1 for s in self.subch if s.flags & SUBCH_DABPLUS))
        given = (max_subch, max_bitrate, max_dabplus)
        self.max_subch, self.max_bitrate, self.max_dabplus = [o if g is None else int(g) for o, g in zip(own, given)]
        self.max_mp2 = sum(1 for s in self.subch if s.flags & SUBCH_MP2) if max_mp2 is None else int(max_mp2)
        if given == (None, None, None) and max_mp2 is None:
            _chk(lib().dabgpu_pipe_create(ctx.h, C.byref(cfg), C.byref(h)), "dabgpu_pipe_create")
        else:
            caps = PipeCaps(self.max_subch, self.max_bitrate, self.max_dabplus, self.max_mp2)
            _chk(lib().dabgpu_pipe_create_caps(ctx.h, C.byref(cfg), C.byref(caps), C.byref(h)),
                 "dabgpu_pipe_create_caps")
        self.h = h
        self.msc_stride = max(24 * self.max_bitrate, 768)
        self.msc_stride = (self.msc_stride + 15) // 16 * 16
        self.msc_stride_packed = self.msc_stride // 8        # bytes per codeword with set_packed
        self.packed = False
        self.fic_packed = False
        self.iq_format = IQ_F32                              # dabgpu_pipe_set_iq_format's default
        # consecutive runs decode concurrently on two back-end streams (dabgpu.h,
        # dabgpu_pipe_sync): outputs alternate between two buffer sets
        self._outs = [(ctx.buf(n_streams * n_frames * 4 * 768), ctx.buf(n_streams * n_frames * 12),
                       ctx.buf(max(1, n_streams * 4 * n_frames * self.max_subch * self.msc_stride)))
                      for _ in range(2)]
        self._run = 0
        self.fic_d, self.crc_d, self.msc_d = self._outs[0]
        self.dp = [s for s in self.subch if s.flags & SUBCH_DABPLUS]
        self.sf_stride = max([110 * (s.bitRate // 8) for s in self.dp] + [16])
        if given != (None, None, None) and self.max_dabplus:
            self.sf_stride = (110 * (self.max_bitrate // 8) + 15) // 16 * 16   # any DAB+ entry the caps allow
        self._sf = []
        if self.max_dabplus:
            # two sets as well: run r's records may still be copied out (fetch) while
            # run r+1's DAB+ layer writes
            nrec = n_streams * 4 * n_frames * self.max_dabplus
            self._sf = [(ctx.buf(nrec * self.sf_stride), ctx.buf(nrec * C.sizeof(Superframe))) for _ in range(2)]
            self.sf_d, self.sfi_d = self._sf[0]
        self._mp2 = []
        if self.max_mp2:
            nrec = n_streams * 4 * n_frames * self.max_mp2
            self._mp2 = [(ctx.buf(nrec * 1152 * 4).zero(), ctx.buf(nrec * MP2_INFO_DTYPE.itemsize)) for _ in range(2)]

        self._pkt = []
        self._ip = []
        self.max_packet = sum(1 for s in self.subch if s.flags & SUBCH_PACKET)
        self.max_group_bytes = PKT_GROUP_BYTES
        if max_packet is not None or max_group_bytes is not None:
            self.packet_caps(self.max_packet if max_packet is None else max_packet, max_group_bytes or 0)
        else:
            self._packet_bufs()
        self._mot = []
        self.max_mot = sum(1 for s in self.subch if s.flags & SUBCH_MOT)
        self.max_body_bytes = MOT_BODY_BYTES
        if max_mot is not None or max_body_bytes is not None:
            self.mot_caps(self.max_mot if max_mot is None else max_mot, max_body_bytes or 0)
        else:
            self._mot_bufs()
        self._pad = []
        self.max_pad = sum(1 for s in self.subch if s.flags & SUBCH_PAD)
        self._pad_bufs()
        self._fic = []                   # the FIC layer's outputs, while fic_caps is on
        self._audio = []
        self.max_audio = sum(1 for s in self.subch if s.flags & SUBCH_AUDIO)
        self._audio_bufs()

    def _audio_bufs(self) -> None:
        for o in self._audio:
            for b in o:
                b.free()
        self._audio = []
        if self.max_audio:
            nrec = self.S * 4 * self.F * self.max_audio
            self._audio = [(self.ctx.buf(nrec * 2304 * 8).zero(), self.ctx.buf(nrec * 4)) for _ in range(2)]

    def audio_caps(self, max_audio: int) -> None:
        """size the audio output layer between runs (dabgpu_pipe_audio_caps): max_audio slots per
        stream (<= max_mp2); the existing slots keep their sinks"""
        _chk(lib().dabgpu_pipe_audio_caps(self.h, int(max_audio)), "dabgpu_pipe_audio_caps")
        self.max_audio = int(max_audio)
        self._audio_bufs()

    def audio(self, download: bool = True):
        """Audio output layer over the frames of this run's mp2() (dabgpu_pipe_audio; audiosink.cpp:
        235-360).  Returns (samples [S, 4F, max_audio, 2304, 2] float32, the first n_out pairs of a
        row valid, n_out [S, 4F, max_audio] int32: 0, 1152 or 2304)."""
        if not self._audio or not hasattr(self, "pcm_d"):
            # max_audio == 0, or no mp2() yet: there are no buffers to hand to the library, which would refuse as well
            e = DabError("dabgpu_pipe_audio: no audio output subchannel in this pipeline" if not self._audio else
                         "dabgpu_pipe_audio: no dabgpu_pipe_mp2 call of this run to consume")
            e.code = -6                  # DABGPU_E_STATE
            raise e
        self.aus_d, self.aun_d = self._audio[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_audio(self.h, self.pcm_d.ptr, self.mp2i_d.ptr, self.aus_d.ptr, self.aun_d.ptr), "dabgpu_pipe_audio")
        if not download:
            return None
        self.sync()
        shape = (self.S, 4 * self.F, self.max_audio)
        return self.aus_d.download(np.float32, shape + (2304, 2)), self.aun_d.download(np.int32, shape)

    def _pad_bufs(self) -> None:
        for o in self._pad:
            for b in o:
                b.free()
        self._pad = []
        if self.max_pad:
            ne, na = self.S * self.max_pad, pad_au_slots(self.F)
            self._pad = [(self.ctx.buf(ne * 4 * na * PAD_LABEL_DTYPE.itemsize), self.ctx.buf(ne * 4 * na * DATAGROUP_DTYPE.itemsize),
                          self.ctx.buf(ne * pad_arena_bytes(self.F)), self.ctx.buf(ne * PAD_RUN_DTYPE.itemsize)) for _ in range(2)]

    def pad_caps(self, max_pad: int) -> None:
        """size the PAD layer between runs (dabgpu_pipe_pad_caps): max_pad slots per stream
        (<= max_dabplus); the existing slots keep their padHandlers"""
        _chk(lib().dabgpu_pipe_pad_caps(self.h, int(max_pad)), "dabgpu_pipe_pad_caps")
        self.max_pad = int(max_pad)
        self._pad_bufs()

    def pad(self, download: bool = True):
        """PAD layer over the AUs of this run's dabplus() (dabgpu_pipe_pad; pad-handler.cpp).
        Returns (labels [S, max_pad, 4 * pad_au_slots(F)] PAD_LABEL_DTYPE -- the first
        run.n_labels of a row are this run's --, groups [S, max_pad, 4 * pad_au_slots(F)]
        DATAGROUP_DTYPE, bytes [S, max_pad, pad_arena_bytes(F)] uint8, run [S, max_pad]
        PAD_RUN_DTYPE)."""
        if not self._pad:                # max_pad == 0: there are no output buffers to hand to the library,
            e = DabError("dabgpu_pipe_pad: no PAD subchannel in this pipeline")   # which would refuse as well
            e.code = -6
            raise e
        self.padl_d, self.padg_d, self.padb_d, self.padr_d = self._pad[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_pad(self.h, self.sf_d.ptr, self.sf_stride, self.sfi_d.ptr, self.padl_d.ptr, self.padg_d.ptr,
                                   self.padb_d.ptr, self.padr_d.ptr), "dabgpu_pipe_pad")
        if not download:
            return None
        self.sync()
        S, NP, ns = self.S, self.max_pad, 4 * pad_au_slots(self.F)
        return (_records(self.padl_d, PAD_LABEL_DTYPE, (S, NP, ns)), _records(self.padg_d, DATAGROUP_DTYPE, (S, NP, ns)),
                self.padb_d.download(np.uint8, (S, NP, pad_arena_bytes(self.F))), _records(self.padr_d, PAD_RUN_DTYPE, (S, NP)))

    def fic_caps(self, on: bool = True) -> None:
        """the FIC layer on (a new database per stream) or off (dabgpu_pipe_fic_caps), between runs"""
        _chk(lib().dabgpu_pipe_fic_caps(self.h, 1 if on else 0), "dabgpu_pipe_fic_caps")
        for o in self._fic:
            for b in o:
                b.free()
        self._fic = []
        if on:
            S = self.S
            self._fic = [(self.ctx.buf(S * FIC_EVENT_SLOTS * FIC_EVENT_DTYPE.itemsize), self.ctx.buf(S * FIC_TABLE_DTYPE.itemsize),
                          self.ctx.buf(S * FIC_RUN_DTYPE.itemsize)) for _ in range(2)]

    def fic(self, want: int = 0, download: bool = True):
        """FIC layer over the FIBs of this run (dabgpu_pipe_fic; fib-processor.cpp).  Returns
        (events [S, FIC_EVENT_SLOTS] FIC_EVENT_DTYPE -- the first run.n_events of a row --,
        table [S] FIC_TABLE_DTYPE, run [S] FIC_RUN_DTYPE)."""
        if not self._fic:                # no layer: there are no output buffers to hand to the library,
            e = DabError("dabgpu_pipe_fic: no FIC layer in this pipeline (fic_caps)")   # which would refuse as well
            e.code = -6
            raise e
        self.fice_d, self.fict_d, self.ficr_d = self._fic[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_fic(self.h, self.fic_d.ptr, self.crc_d.ptr, int(want), self.fice_d.ptr, self.fict_d.ptr,
                                   self.ficr_d.ptr), "dabgpu_pipe_fic")
        if not download:
            return None
        self.sync()
        return (_records(self.fice_d, FIC_EVENT_DTYPE, (self.S, FIC_EVENT_SLOTS)), _records(self.fict_d, FIC_TABLE_DTYPE, (self.S,)),
                _records(self.ficr_d, FIC_RUN_DTYPE, (self.S,)))

    def fic_db(self, stream: int) -> np.ndarray:
        """one stream's database, a FIC_DB_DTYPE record (dabgpu_pipe_fic_db)"""
        db = np.zeros(1, FIC_DB_DTYPE)
        _chk(lib().dabgpu_pipe_fic_db(self.h, int(stream), _p(db)), "dabgpu_pipe_fic_db")
        return db[0]

    def fic_clear(self, stream: int = -1) -> None:
        """clearEnsemble for one stream's database, -1 for all (dabgpu_pipe_fic_clear)"""
        _chk(lib().dabgpu_pipe_fic_clear(self.h, int(stream)), "dabgpu_pipe_fic_clear")

    def _mot_bufs(self) -> None:
        for o in self._mot:
            for b in o:
                b.free()
        self._mot = []
        if self.max_mot:
            ne, gs = self.S * self.max_mot, pkt_group_slots(self.F, self.max_bitrate)
            self._mot = [(self.ctx.buf(ne * mot_arena_bytes(gs, self.max_body_bytes)),
                          self.ctx.buf(ne * gs * MOT_OBJECT_DTYPE.itemsize),
                          self.ctx.buf(ne * MOT_RUN_DTYPE.itemsize)) for _ in range(2)]

    def mot_caps(self, max_mot: int, max_body_bytes: int = 0) -> None:
        """size the MOT layer between runs (dabgpu_pipe_mot_caps): max_mot slots per stream
        (<= max_packet), bodies of at most max_body_bytes (0: MOT_BODY_BYTES); the existing
        slots keep their motHandlers"""
        _chk(lib().dabgpu_pipe_mot_caps(self.h, int(max_mot), int(max_body_bytes)), "dabgpu_pipe_mot_caps")
        self.max_mot, self.max_body_bytes = int(max_mot), int(max_body_bytes) or MOT_BODY_BYTES
        self._mot_bufs()

    def mot(self, download: bool = True):
        """MOT layer over the groups of this run's packet() (dabgpu_pipe_mot; mot-data.cpp:
        679-728 in header mode).  Returns (bytes [S, max_mot, arena] uint8, objects [S, max_mot,
        slots] MOT_OBJECT_DTYPE -- the first run.n_objects of a row are this run's --, run
        [S, max_mot] MOT_RUN_DTYPE)."""
        if not self._mot:                # max_mot == 0: there are no output buffers to hand to the library,
            e = DabError("dabgpu_pipe_mot: no MOT subchannel in this pipeline")   # which would refuse as well
            e.code = -6                  # DABGPU_E_STATE
            raise e
        self.motb_d, self.moto_d, self.motr_d = self._mot[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_mot(self.h, self.motb_d.ptr, self.moto_d.ptr, self.motr_d.ptr), "dabgpu_pipe_mot")
        if not download:
            return None
        self.sync()
        S, NM, gs = self.S, self.max_mot, pkt_group_slots(self.F, self.max_bitrate)
        return (self.motb_d.download(np.uint8, (S, NM, mot_arena_bytes(gs, self.max_body_bytes))),
                _records(self.moto_d, MOT_OBJECT_DTYPE, (S, NM, gs)), _records(self.motr_d, MOT_RUN_DTYPE, (S, NM)))

    def ip(self, download: bool = True):
        """IP layer over the groups of this run's packet() (dabgpu_pipe_ip; ip-datahandler.cpp:
        40-127), for the entries flagged SUBCH_PACKET | SUBCH_IP.  Returns (bytes [S, max_packet,
        arena] uint8, results [S, max_packet, slots] IP_RESULT_DTYPE -- the first n_groups of a row
        of this run's packet() are this run's --, run [S, max_packet] IP_RUN_DTYPE), indexed by
        packet slot; the slot of an entry that is not flagged has an all-zero run."""
        if not self._pkt:                # max_packet == 0: the library refuses (DABGPU_E_STATE) before it writes
            _chk(lib().dabgpu_pipe_ip(self.h, self.fic_d.ptr, self.fic_d.ptr, self.fic_d.ptr), "dabgpu_pipe_ip")
            raise DabError("dabgpu_pipe_ip accepted a pipeline without packet slots")
        if not self._ip:
            ne, gs = self.S * self.max_packet, pkt_group_slots(self.F, self.max_bitrate)
            oa = ip_arena_bytes(gs, pkt_arena_bytes(self.F, self.max_bitrate, self.max_group_bytes))
            self._ip = [(self.ctx.buf(ne * oa), self.ctx.buf(ne * gs * IP_RESULT_DTYPE.itemsize),
                         self.ctx.buf(ne * IP_RUN_DTYPE.itemsize)) for _ in range(2)]
        self.ipb_d, self.ipo_d, self.ipr_d = self._ip[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_ip(self.h, self.ipb_d.ptr, self.ipo_d.ptr, self.ipr_d.ptr), "dabgpu_pipe_ip")
        if not download:
            return None
        self.sync()
        S, NP, gs = self.S, self.max_packet, pkt_group_slots(self.F, self.max_bitrate)
        oa = ip_arena_bytes(gs, pkt_arena_bytes(self.F, self.max_bitrate, self.max_group_bytes))
        return (self.ipb_d.download(np.uint8, (S, NP, oa)), _records(self.ipo_d, IP_RESULT_DTYPE, (S, NP, gs)),
                _records(self.ipr_d, IP_RUN_DTYPE, (S, NP)))

    def ip_state(self, stream: int) -> np.ndarray:
        """one stream's ip_dataHandler counters by packet slot, [max_packet] IP_STATE_DTYPE (dabgpu_pipe_ip_state)"""
        st = np.zeros(max(1, self.max_packet), IP_STATE_DTYPE)
        _chk(lib().dabgpu_pipe_ip_state(self.h, int(stream), _p(st)), "dabgpu_pipe_ip_state")
        return st[:self.max_packet]

    def _packet_bufs(self) -> None:
        for o in self._pkt + self._ip:
            for b in o:
                b.free()
        self._pkt = []
        self._ip = []                    # (allocated by the first ip() call)
        if self.max_packet:
            ne = self.S * self.max_packet
            self._pkt = [(self.ctx.buf(ne * pkt_arena_bytes(self.F, self.max_bitrate, self.max_group_bytes)),
                          self.ctx.buf(ne * pkt_group_slots(self.F, self.max_bitrate) * DATAGROUP_DTYPE.itemsize),
                          self.ctx.buf(ne * PACKET_RUN_DTYPE.itemsize),
                          self.ctx.buf(ne * 4 * self.F * PACKET_INFO_DTYPE.itemsize)) for _ in range(2)]

    def packet_caps(self, max_packet: int, max_group_bytes: int = 0) -> None:
        """size the packet-mode layer between runs (dabgpu_pipe_packet_caps): max_packet slots
        per stream, groups of at most max_group_bytes (0: PKT_GROUP_BYTES); the existing
        entries keep their assembler state"""
        _chk(lib().dabgpu_pipe_packet_caps(self.h, int(max_packet), int(max_group_bytes)), "dabgpu_pipe_packet_caps")
        self.max_packet, self.max_group_bytes = int(max_packet), int(max_group_bytes) or PKT_GROUP_BYTES
        self._packet_bufs()

    def packet(self, download: bool = True):
        """packet-mode data layer over the CIFs of the last run() (dabgpu_pipe_packet;
        msc-datagroup.cpp:221-319, mot-databuilder.cpp:37-95).  Returns (bytes [S, max_packet,
        arena] uint8, groups [S, max_packet, slots] DATAGROUP_DTYPE -- the first run.n_groups of a
        row are this run's --, run [S, max_packet] PACKET_RUN_DTYPE, info [S, 4F, max_packet]
        PACKET_INFO_DTYPE)."""
        if not self._pkt:                # max_packet == 0: the library refuses (DABGPU_E_STATE) before it writes
            _chk(lib().dabgpu_pipe_packet(self.h, self.fic_d.ptr, self.fic_d.ptr, self.fic_d.ptr, self.fic_d.ptr),
                 "dabgpu_pipe_packet")
            raise DabError("dabgpu_pipe_packet accepted a pipeline without packet slots")
        self.pkb_d, self.pkg_d, self.pkr_d, self.pki_d = self._pkt[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_packet(self.h, self.pkb_d.ptr, self.pkg_d.ptr, self.pkr_d.ptr, self.pki_d.ptr),
             "dabgpu_pipe_packet")
        if not download:
            return None
        self.sync()
        S, NP = self.S, self.max_packet

        def rec(buf, dtype, shape):
            raw = buf.download(np.uint8, int(np.prod(shape)) * dtype.itemsize)
            return np.frombuffer(raw.tobytes(), dtype=dtype).reshape(shape)
        return (self.pkb_d.download(np.uint8, (S, NP, pkt_arena_bytes(self.F, self.max_bitrate, self.max_group_bytes))),
                rec(self.pkg_d, DATAGROUP_DTYPE, (S, NP, pkt_group_slots(self.F, self.max_bitrate))),
                rec(self.pkr_d, PACKET_RUN_DTYPE, (S, NP)), rec(self.pki_d, PACKET_INFO_DTYPE, (S, 4 * self.F, NP)))

    def acquire(self, iq: DevBuf, stride: int, start: Sequence[int], n_avail: Sequence[int]) -> None:
        st = np.asarray(start, dtype=np.int64)
        na = np.asarray(n_avail, dtype=np.int64)
        _chk(lib().dabgpu_pipe_acquire(self.h, iq.ptr, stride, _p(st), _p(na)), "dabgpu_pipe_acquire")

    def run(self, iq: DevBuf, stride: int, n_avail: Sequence[int], download: bool = True, partial: bool = False):
        """one dabgpu_pipe_run; partial=True accepts a run in which a stream ran out of
        samples (DABGPU_E_STATE: its decoded frames are still delivered)"""
        na = np.asarray(n_avail, dtype=np.int64)
        valid = np.zeros((self.S, 4 * self.F), dtype=np.uint8)
        self.fic_d, self.crc_d, self.msc_d = self._outs[self._run & 1]
        self._run += 1
        ms = self.msc_stride_packed if self.packed else self.msc_stride
        rc = lib().dabgpu_pipe_run(self.h, iq.ptr, stride, _p(na), self.fic_d.ptr, self.crc_d.ptr,
                                   self.msc_d.ptr if self.max_subch else None, ms, _p(valid))
        if not (partial and rc == -6):
            _chk(rc, "dabgpu_pipe_run")
        if not download:
            return valid
        self.sync()
        fic = self.fic_d.download(np.uint8, (self.S, self.F, 4, 96 if self.fic_packed else 768))
        crc = self.crc_d.download(np.uint8, (self.S, self.F, 12))
        msc = self.msc_d.download(np.uint8, (self.S, 4 * self.F, self.max_subch, ms)) if self.max_subch else None
        return fic, crc, msc, valid

    def set_subch(self, stream: int, subs: Sequence[Subch]) -> None:
        """replace the subchannel table of `stream` (-1: of every stream) for the runs that
        follow (dabgpu_pipe_set_subch): unchanged entries go on, the others deliver from the
        stream's current CIF + 16.  Call dabplus() for the last run before it."""
        subs = list(subs)
        arr = (Subch * max(1, len(subs)))(*subs)
        _chk(lib().dabgpu_pipe_set_subch(self.h, int(stream), C.cast(arr, C.c_void_p), len(subs)),
             "dabgpu_pipe_set_subch")

    def get_subch(self, stream: int):
        """(the stream's table as a list of Subch, since_cif of each entry)"""
        arr = (Subch * max(1, self.max_subch))()
        n = C.c_int32()
        since = np.zeros(max(1, self.max_subch), np.int64)
        _chk(lib().dabgpu_pipe_get_subch(self.h, int(stream), C.cast(arr, C.c_void_p), C.byref(n), _p(since)),
             "dabgpu_pipe_get_subch")
        return [Subch(a.startAddr, a.length, a.bitRate, a.protLevel, a.uepFlag, a.flags) for a in arr[:n.value]], \
            [int(x) for x in since[:n.value]]

    def msc_entry_valid(self) -> np.ndarray:
        """[S, 4F, max_subch] uint8 of the last run: the stream delivered the CIF and it is
        past the entry's own 16-CIF warm-up (dabgpu_pipe_msc_entry_valid)"""
        v = np.zeros((self.S, 4 * self.F, max(1, self.max_subch)), np.uint8)
        _chk(lib().dabgpu_pipe_msc_entry_valid(self.h, _p(v)), "dabgpu_pipe_msc_entry_valid")
        return v[:, :, :self.max_subch]

    def set_dabplus_compact(self, on: bool = True) -> None:
        """compact superframe bytes (dabgpu_pipe_set_dabplus_compact): dabplus() then returns
        bytes [S, n_dabplus, sf_slots, sf_stride], the run's superframes in CIF order, and
        each record's `reserved` is its slot"""
        _chk(lib().dabgpu_pipe_set_dabplus_compact(self.h, int(on)), "dabgpu_pipe_set_dabplus_compact")
        self.dp_compact = bool(on)

    @property
    def sf_slots(self) -> int:
        return (4 * self.F + 4) // 5 + 1                  # DABGPU_SF_SLOTS

    def dabplus(self, download: bool = True):
        """DAB+ superframe layer over the CIFs of the last run() (mp4processor.cpp:107-292).
        Returns (info [S, 4F, n_dabplus] Superframe records, bytes [S, 4F, n_dabplus, sf_stride]
        -- or [S, n_dabplus, sf_slots, sf_stride] with set_dabplus_compact)."""
        self.sf_d, self.sfi_d = self._sf[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_dabplus(self.h, self.sf_d.ptr, self.sf_stride, self.sfi_d.ptr), "dabgpu_pipe_dabplus")
        if not download:
            return None
        self.sync()
        nd = self.max_dabplus
        raw = self.sfi_d.download(np.uint8, self.S * 4 * self.F * nd * C.sizeof(Superframe))
        info = np.frombuffer(raw.tobytes(), dtype=SUPERFRAME_DTYPE).reshape(self.S, 4 * self.F, nd)
        if getattr(self, "dp_compact", False):
            sf = self.sf_d.download(np.uint8, (self.S, nd, self.sf_slots, self.sf_stride))
        else:
            sf = self.sf_d.download(np.uint8, (self.S, 4 * self.F, nd, self.sf_stride))
        return info, sf

    def mp2(self, download: bool = True):
        """MPEG layer II layer over the CIFs of the last run() (dabgpu_pipe_mp2; mp2processor.cpp:
        365-617).  Returns (pcm [S, 4F, max_mp2, 1152, 2] int16, valid where info.status == 2,
        info [S, 4F, max_mp2] MP2_INFO_DTYPE records)."""
        if not self._mp2:                # max_mp2 == 0: the library refuses (DABGPU_E_STATE) before it writes
            _chk(lib().dabgpu_pipe_mp2(self.h, self.fic_d.ptr, self.crc_d.ptr), "dabgpu_pipe_mp2")
            raise DabError("dabgpu_pipe_mp2 accepted a pipeline without layer II slots")
        self.pcm_d, self.mp2i_d = self._mp2[(self._run - 1) & 1]
        _chk(lib().dabgpu_pipe_mp2(self.h, self.pcm_d.ptr, self.mp2i_d.ptr), "dabgpu_pipe_mp2")
        if not download:
            return None
        self.sync()
        shape = (self.S, 4 * self.F, self.max_mp2)
        raw = self.mp2i_d.download(np.uint8, int(np.prod(shape)) * MP2_INFO_DTYPE.itemsize)
        return (self.pcm_d.download(np.int16, shape + (1152, 2)),
                np.frombuffer(raw.tobytes(), dtype=MP2_INFO_DTYPE).reshape(shape))

    STAGES = ("prs_sync", "block0", "demod", "fic", "msc_acs", "msc_traceback", "dabplus")

    def sync(self) -> None:
        """wait for every stage of the last run (channel decoding runs on the
        pipeline's own stream, overlapping the next run's front end)"""
        _chk(lib().dabgpu_pipe_sync(self.h), "dabgpu_pipe_sync")

    def set_profiling(self, on=True) -> None:
        """True/1: time the last run; 2: accumulate over every run from now on; 3: as 2
        with every stage run alone on the device (roofline timing); False/0: off"""
        mode = 0 if on is False else 1 if on is True else int(on)
        _chk(lib().dabgpu_pipe_set_profiling(self.h, mode), "set_profiling")

    def timing(self) -> dict:
        """per-stage kernel milliseconds and launch counts (last run, or summed since
        set_profiling(2))"""
        ms = np.zeros(len(self.STAGES), np.float32)
        n = np.zeros(len(self.STAGES), np.int32)
        _chk(lib().dabgpu_pipe_timing(self.h, _p(ms), _p(n)), "timing")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.STAGES)}

    def state(self, s: int) -> StreamState:
        o = StreamState()
        _chk(lib().dabgpu_pipe_state(self.h, s, C.byref(o)), "dabgpu_pipe_state")
        return o

    def frame_info(self):
        """[S][F] FrameInfo records of the last run"""
        n = self.S * self.F
        fi = (FrameInfo * n)()
        _chk(lib().dabgpu_pipe_frame_info(self.h, C.cast(fi, C.c_void_p)), "dabgpu_pipe_frame_info")
        return [list(fi)[s * self.F:(s + 1) * self.F] for s in range(self.S)]

    def control(self, op: int, stream: int = -1) -> None:
        """ofdmProcessor's reset / coarseCorrectorOn/Off / set_scanMode (dabgpu_pipe_control)"""
        _chk(lib().dabgpu_pipe_control(self.h, stream, op), "dabgpu_pipe_control")

    def frames(self):
        n = self.S * self.F
        fr = (Frame * n)()
        si = np.zeros(n, dtype=np.int32)
        _chk(lib().dabgpu_pipe_frames(self.h, C.cast(fr, C.c_void_p), _p(si)), "dabgpu_pipe_frames")
        return list(fr), si.reshape(self.S, self.F)

    def set_packed(self, on=True) -> None:
        """output format of the following runs (dabgpu_pipe_set_packed): True / PACK_MSC:
        MSC 8 bits per byte, msb first (packbits order) instead of one bit per byte -- run()
        then returns msc [S, 4F, n_subch, msc_stride_packed] bytes; | PACK_FIC: the FIC as
        FIB bytes, fic [S, F, 4, 96]"""
        m = PACK_MSC if on is True else 0 if on is False else int(on)
        _chk(lib().dabgpu_pipe_set_packed(self.h, m), "dabgpu_pipe_set_packed")
        self.packed = bool(m & PACK_MSC)
        self.fic_packed = bool(m & PACK_FIC)

    def acquire_wait(self) -> None:
        """wait for a background null search in flight and apply it (dabgpu_pipe_acquire_wait)"""
        _chk(lib().dabgpu_pipe_acquire_wait(self.h), "dabgpu_pipe_acquire_wait")

    def set_display_token(self, token: int) -> None:
        """the symbol (1..75) the display feed keeps (ofdmDecoder::set_displayToken)"""
        _chk(lib().dabgpu_pipe_set_display_token(self.h, int(token)), "dabgpu_pipe_set_display_token")

    def set_iq_format(self, fmt: int) -> None:
        """sample format of the streams acquire() / run() read: IQ_F32 (default), IQ_S16
        (.sdr PCM16) or IQ_U8 (.raw), converted exactly in the kernels' loads
        (dabgpu_pipe_set_iq_format); strides and n_avail stay in samples"""
        _chk(lib().dabgpu_pipe_set_iq_format(self.h, int(fmt)), "dabgpu_pipe_set_iq_format")
        self.iq_format = int(fmt)

    def fetch(self, dst: "HostBuf", src: DevBuf, nbytes: int, dst_off: int = 0) -> None:
        """asynchronous copy of an output of the last run to pinned host memory, behind
        that run's channel decoding (dabgpu_pipe_fetch)"""
        _chk(lib().dabgpu_pipe_fetch(self.h, C.c_void_p(dst.ptr.value + dst_off), src.ptr, nbytes),
             "dabgpu_pipe_fetch")

    def set_display(self, on: bool = True) -> None:
        """keep symbol 2's display carriers of every decoded frame (dabgpu_pipe_set_display)"""
        _chk(lib().dabgpu_pipe_set_display(self.h, int(on)), "dabgpu_pipe_set_display")

    def iq_display(self, stream: int, frame: int) -> np.ndarray:
        """processToken's iqBuffer values (ofdm-decoder.cpp:197-205) of (stream, frame) of
        the last run: complex64 [1536]"""
        out = np.zeros((K, 2), np.float32)
        _chk(lib().dabgpu_pipe_iq_display(self.h, stream, frame, _p(out)), "dabgpu_pipe_iq_display")
        return out[:, 0] + 1j * out[:, 1]

    def softbits(self) -> np.ndarray:
        """the soft-bit ring of the last run as [stream][slot][75][3072] ibits rows (the ring
        holds ibits + 127 as bytes, dabgpu.h dabgpu_pipe_softbits)"""
        p, r = C.c_void_p(), C.c_int32()
        _chk(lib().dabgpu_pipe_softbits(self.h, C.byref(p), C.byref(r)), "softbits")
        n = self.S * r.value * NSYM * SYMBITS
        raw = np.empty(n, dtype=np.uint8)
        _chk(lib().dabgpu_memcpy_d2h(self.ctx.h, _p(raw), p, raw.nbytes), "d2h")
        return (raw.astype(np.int16) - 127).reshape(self.S, r.value, NSYM, SYMBITS)

    def close(self) -> None:
        if self.h:
            for o in self._outs + self._sf + self._mp2 + self._pkt + self._ip + self._mot + self._pad + self._fic + self._audio:
                for b in o:
                    b.free()
            lib().dabgpu_pipe_destroy(self.h)
            self.h = None
