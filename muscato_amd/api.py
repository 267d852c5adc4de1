"""Host-side binding of the hot path: utils.Config mirror + one Engine per GPU.

The reference's interface for this path is the pair of executables
``muscato_screen config.json`` / ``muscato_confirm config.json k``
(cmd/muscato/main.go:306-316, 387-420) driven by ``utils.Config``
(utils/config.go:10-101).  ``Config`` keeps the same field names, JSON form
and defaults; ``Engine`` is the in-process replacement of the two executables
plus the sort between them, through the C ABI of include/muscato_hip.h.
"""
from __future__ import annotations

import ctypes
import json
from dataclasses import dataclass, field, asdict
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _cov, _lib, _sam


class MuscatoError(RuntimeError):
    pass


@dataclass
class DbTextInfo:
    """musc_db_text_info: what Engine.load_db_text found in the gene file."""
    n_targets: int
    n_bases: int
    n_odd: int               # target bytes that are none of A C G T X
    first_odd_target: int
    n_text_bytes: int
    n_chunks: int            # data chunks of the stream (0 for plain text)
    ms_decode: float
    ms_parse: float


@dataclass
class TargetsPrepInfo:
    """musc_targets_prep_info: what Engine.prep_targets made of the raw target file."""
    n_lines: int
    n_records: int           # kept records (one strand)
    n_targets: int           # lines of the sequence text: both strands with rev
    n_dropped: int           # FASTA records without bases
    stop_line: int           # text format: the first stop line, 2**64 - 1 when the input ran out
    n_subx: int              # bytes that subx changed
    n_seq_bytes: int
    n_id_bytes: int
    ms: float


@dataclass
class Config:
    """utils/config.go:10-101 -- same names; defaults of cmd/muscato/main.go:833-904."""
    ReadFileName: str = ""
    GeneFileName: str = ""
    GeneIdFileName: str = ""
    ResultsFileName: str = ""
    Windows: List[int] = field(default_factory=list)
    WindowWidth: int = 0
    BloomSize: int = 0
    NumHash: int = 0
    PMatch: float = 0.0
    MinDinuc: int = 0
    TempDir: str = ""
    LogDir: str = ""
    MinReadLength: int = 0
    MaxReadLength: int = 0
    MaxMatches: int = 0
    MaxConfirmProcs: int = 0
    MMTol: int = 0
    MatchMode: str = ""
    SortPar: int = 0
    SortTemp: str = ""
    SortMem: str = ""
    NoCleanTemp: bool = False
    CPUProfile: bool = False
    MaxMismatch: int = -1  # addition: absolute mismatch budget (overrides PMatch when >= 0)
    # addition: most target bases indexed at once.  A value > 0 is applied to the Engine by match / build_index_for
    # (Engine.set_partition_bases); 0 leaves the engine's setting, which is automatic unless set_partition_bases changed it
    DbPartitionBases: int = 0

    @classmethod
    def from_json(cls, text) -> "Config":
        d = json.loads(text) if isinstance(text, (str, bytes)) else dict(text)
        c = cls()
        for k, v in d.items():
            if hasattr(c, k) and v is not None:
                setattr(c, k, v)
        return c

    def to_json(self) -> str:
        return json.dumps(asdict(self))

    def with_defaults(self) -> "Config":
        """checkArgs (cmd/muscato/main.go:833-904) for the fields the hot path reads."""
        c = Config(**asdict(self))
        if not c.Windows:
            raise MuscatoError("Windows not provided")
        if c.WindowWidth == 0:
            raise MuscatoError("WindowWidth not provided")
        if c.MaxReadLength == 0:
            raise MuscatoError("MaxReadLength not provided")
        if c.BloomSize == 0:
            c.BloomSize = 4 * 1000 * 1000 * 1000
        if c.NumHash == 0:
            c.NumHash = 20
        if c.PMatch == 0:
            c.PMatch = 1.0
        if c.MaxMatches == 0:
            c.MaxMatches = 1000 * 1000
        if c.MaxConfirmProcs == 0:
            c.MaxConfirmProcs = 3
        if c.MatchMode == "":
            c.MatchMode = "best"
        if c.MatchMode not in ("best", "first"):
            raise MuscatoError("MatchMode must be 'first' or 'best'")
        if c.ResultsFileName == "":
            c.ResultsFileName = "results.txt"
        if c.DbPartitionBases < 0:
            raise MuscatoError("DbPartitionBases must be >= 0")
        return c

    def to_params(self, apply_mmtol: bool, skip_block_check: bool = False, n_shards: int = 1) -> _lib.MuscParams:
        """n_shards > 1: this context sees one of n_shards contiguous slices of the reads, so a
        (window,key) block is split across contexts and the MaxMatches check must use
        MaxMatches / n_shards (include/muscato_hip.h, musc_params.n_shards)."""
        c = self.with_defaults()
        if len(c.Windows) > _lib.MUSC_MAX_WINDOWS:
            raise MuscatoError("at most %d windows are supported" % _lib.MUSC_MAX_WINDOWS)
        p = _lib.MuscParams()
        p.n_windows = len(c.Windows)
        for i, w in enumerate(c.Windows):
            p.windows[i] = int(w)
        p.window_width = int(c.WindowWidth)
        p.pmatch = float(c.PMatch)
        p.min_dinuc = int(c.MinDinuc)
        p.max_read_length = int(c.MaxReadLength)
        p.max_matches = int(c.MaxMatches)
        p.match_mode = 1 if c.MatchMode == "first" else 0
        p.mmtol = int(c.MMTol)
        p.apply_mmtol = 1 if apply_mmtol else 0
        p.max_mismatch_p1 = c.MaxMismatch + 1 if c.MaxMismatch >= 0 else 0
        p.skip_block_check = 1 if skip_block_check else 0
        p.n_shards = max(1, int(n_shards))
        return p


def concat(seqs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """list of ASCII sequences -> (uint8 buffer, uint64 offsets[n+1])."""
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(seqs) + b"\0" * 8, dtype=np.uint8).copy()
    return buf, off


_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def pack_2bit(buf: np.ndarray, nbases: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """ASCII bases -> the packed ABI form: 2 bits per base (A0 C1 G2 T3), 4 bases per
    byte little-endian, plus a 1-bit-per-base X mask (None if there is no X)."""
    codes = _CODE[buf[:nbases]]
    isx = codes == 255
    codes = np.where(isx, 0, codes).astype(np.uint8)
    pad = (-nbases) % 4
    c4 = np.concatenate([codes, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    packed = (c4[:, 0] | (c4[:, 1] << 2) | (c4[:, 2] << 4) | (c4[:, 3] << 6)).astype(np.uint8)
    mask = np.packbits(isx, bitorder="little") if isx.any() else None
    return packed, mask


def _host_ptr(data) -> Tuple[Optional[int], int]:
    """Host bytes -> (their address, or None when there are none; their number).  `data` owns the memory: the caller
    holds it across the call."""
    buf = np.frombuffer(data, dtype=np.uint8)
    return (buf.ctypes.data if len(buf) else None), len(buf)


def _array(p, count: int) -> np.ndarray:
    """A copy of `count` elements at the typed pointer `p`; a count of 0 does not look at the pointer."""
    return np.ctypeslib.as_array(p, shape=(count,)).copy() if count else np.zeros(0, dtype=p._type_)


def _plain(s: ctypes.Structure, cls):
    """A struct of the library as the dataclass `cls` of its fields (all but `reserved`): Python ints and floats."""
    return cls(**{k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"})


class Engine:
    """One context per GPU: resident target database + index, resident reads, match()."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self._lib.musc_init(int(device), ctypes.byref(h))
        if rc != 0:
            raise MuscatoError("musc_init failed: %s" % self._lib.musc_last_error(None).decode())
        self._h = h
        self.device = device
        self.n_targets = 0
        self.n_reads = 0
        self._res_nlines = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.musc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise MuscatoError("%s failed (%d): %s" % (what, rc, self._lib.musc_last_error(self._h).decode()))

    def _call(self, name: str, *args) -> None:
        """The library's `name(ctx, *args)`, checked: the name that is called is the name that is reported."""
        self._check(getattr(self._lib, name)(self._h, *args), name)

    def _sized(self, fill, skip_empty: bool = False) -> bytes:
        """Size, then fill: `fill(dst, capacity, &nbytes)` once with a NULL dst for the size, once more into a host buffer
        of that size (of one byte when the size is 0; skip_empty: no second call then) -> the bytes the second call
        reports."""
        n = ctypes.c_uint64()
        fill(None, 0, ctypes.byref(n))
        if skip_empty and not n.value:
            return b""
        out = np.empty(max(n.value, 1), dtype=np.uint8)
        fill(out.ctypes.data, n.value, ctypes.byref(n))
        return out[:n.value].tobytes()

    def _take_u32(self, *arrays) -> List[np.ndarray]:
        """Copies of uint32 arrays the library malloc'ed, each given as (pointer, count); every one of them is freed,
        whatever happens."""
        try:
            return [_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), int(n)) for p, n in arrays]
        finally:
            for p, _ in arrays:
                self._lib.musc_free_u32(ctypes.cast(p, ctypes.c_void_p))

    def _ms_pair(self, name: str) -> Tuple[float, float]:
        """The two HIP-event times of a `*_last_ms` call."""
        a, b = ctypes.c_float(), ctypes.c_float()
        self._call(name, ctypes.byref(a), ctypes.byref(b))
        return float(a.value), float(b.value)

    def _packed(self, name: str, seqs: Sequence[bytes]) -> int:
        """`seqs` through the packed loader `name` (2 bits a base, an X mask when there is an X) -> their number."""
        buf, off = concat(seqs)
        packed, mask = pack_2bit(buf, int(off[-1]))
        packed = np.concatenate([packed, np.zeros(8, np.uint8)])
        self._call(name, packed.ctypes.data, mask.ctypes.data if mask is not None else None, off.ctypes.data, len(off) - 1)
        return len(off) - 1

    # ---- database (gene number = index in the list = line index of GeneFileName)
    def reload_env(self) -> None:
        """Re-read the MUSC_* knobs (the library reads them once, at musc_init).
        The rule: every MUSC_* knob is latched when the context is made.  Setting or clearing one in the environment of
        a live Engine changes nothing until this call, which latches all of them again -- except MUSC_BATCH_READS, which
        keeps its value of musc_init, and MUSC_RCCL_LIB, which is read once per process."""
        self._call("musc_reload_env")

    def load_targets(self, seqs: Sequence[bytes]) -> None:
        buf, off = concat(seqs)
        self.load_targets_arrays(buf, off)

    def load_targets_arrays(self, buf: np.ndarray, off: np.ndarray) -> None:
        self._call("musc_db_load_ascii", buf.ctypes.data, off.ctypes.data, len(off) - 1, 0)
        self.n_targets = len(off) - 1

    def load_targets_device(self, seqs_ptr: int, off_ptr: int, nseq: int) -> None:
        self._call("musc_db_load_ascii", seqs_ptr, off_ptr, nseq, 1)
        self.n_targets = nseq

    def load_targets_packed(self, seqs: Sequence[bytes]) -> None:
        self.n_targets = self._packed("musc_db_load_packed", seqs)

    def sz_decode(self, data: bytes) -> bytes:
        """A framed snappy stream decoded on the GPU (musc_sz_decode)."""
        sp, n = _host_ptr(data)
        return self._sized(lambda dst, cap, nout: self._call("musc_sz_decode", sp, n, dst, cap, 0, nout))

    def load_db_text(self, data, framed: int = -1, on_device: bool = False) -> "DbTextInfo":
        """The raw bytes of a gene file -- a framed snappy stream or plain text, one target per line up to its first
        tab -- decoded, split and packed on the GPU (musc_db_load_text).  data: bytes, or (on_device) a pair
        (device pointer, nbytes) of plain text at any alignment.  framed: 1, 0, or -1 to go by the stream identifier."""
        ptr, nbytes = data if on_device else _host_ptr(data)
        info = _lib.MuscDbTextInfo()
        self.n_targets = 0
        self._call("musc_db_load_text", ptr, int(nbytes), 1 if on_device else 0, int(framed), ctypes.byref(info))
        self.n_targets = int(info.n_targets)
        return _plain(info, DbTextInfo)

    # ---- target preparation on the device (musc_targets_prep*, musc_sz_frame)
    def prep_targets(self, data, fasta: bool, rev: bool, on_device: bool = False) -> "TargetsPrepInfo":
        """The raw bytes of a target file -- FASTA, or id<TAB>sequence text -- prepared on the GPU: the sequence text and
        the id text stay resident (prepared_text, load_db_prepared) until the next call, free_prepared or close.  data:
        bytes, or (on_device) a pair (device pointer, nbytes) at any alignment."""
        ptr, nbytes = data if on_device else _host_ptr(data)
        info = _lib.MuscTargetsPrepInfo()
        self._prep_bytes = None
        self._call("musc_targets_prep", ptr, int(nbytes), 1 if on_device else 0, int(fasta), int(rev), ctypes.byref(info))
        self._prep_bytes = (int(info.n_seq_bytes), int(info.n_id_bytes))
        return _plain(info, TargetsPrepInfo)

    def prepared_text(self, which: int, off: int = 0, nbytes: Optional[int] = None) -> bytes:
        """Bytes [off, off + nbytes) of a prepared text (which: 0 sequences, 1 ids); nbytes None: to the text's end."""
        if nbytes is None:
            have = getattr(self, "_prep_bytes", None)
            if have is None or which not in (0, 1):
                raise MuscatoError("prepared_text: no prepared text (prep_targets first)" if have is None else "prepared_text: which must be 0 or 1")
            nbytes = max(have[which] - int(off), 0)
        out = np.empty(max(int(nbytes), 1), dtype=np.uint8)
        self._call("musc_targets_prep_text", int(which), int(off), int(nbytes), out.ctypes.data, 0)
        return out[:int(nbytes)].tobytes()

    def load_db_prepared(self) -> "DbTextInfo":
        """The resident sequence text becomes the database (musc_targets_prep_load); the prepared texts stay."""
        info = _lib.MuscDbTextInfo()
        self.n_targets = 0
        self._call("musc_targets_prep_load", ctypes.byref(info))
        self.n_targets = int(info.n_targets)
        return _plain(info, DbTextInfo)

    def free_prepared(self) -> None:
        self._prep_bytes = None
        self._call("musc_targets_prep_free")

    def _sz_write(self, name: str, data: bytes) -> bytes:
        # (a stream is never empty -- its size, or bound, is 10 + 8 * chunks + nbytes -- so _sized's one-byte rule is idle)
        sp, n = _host_ptr(data)
        return self._sized(lambda dst, cap, nout: self._call(name, sp, n, 0, dst, cap, 0, nout))

    def sz_frame(self, data: bytes) -> bytes:
        """`data` as a framed snappy stream of uncompressed chunks, made on the GPU (musc_sz_frame)."""
        return self._sz_write("musc_sz_frame", data)

    def sz_compress(self, data: bytes) -> bytes:
        """`data` as a framed snappy stream of compressed chunks, made on the GPU (musc_sz_compress): the bytes of the
        host writer under MUSC_SZ_WRITE=compressed."""
        return self._sz_write("musc_sz_compress", data)

    def prepared_sz(self, which: int, compressed: bool) -> bytes:
        """A resident prepared text (which: 0 sequences, 1 ids) as a framed snappy stream, made where the text lies
        (musc_targets_prep_sz): sz_compress's bytes of it, or sz_frame's."""
        return self._sized(lambda dst, cap, nout: self._call("musc_targets_prep_sz", int(which), int(bool(compressed)), dst, cap, 0, nout))

    def build_index(self, window_width: int) -> None:
        self._call("musc_db_build_index", int(window_width))

    def build_index_for(self, cfg: "Config", max_read_len: int = 0) -> None:
        """Build the index match() will pick for `cfg` (context buckets when the run fits them; with several
        partitions, the first one's)."""
        p = cfg.to_params(True)
        self._apply_partition_bases(cfg)
        self._call("musc_db_build_index_for", ctypes.byref(p), int(max_read_len))

    def set_partition_bases(self, max_bases: int) -> None:
        """Most target bases indexed at once (musc_db_set_partition_bases): the database is matched in partitions of
        whole targets and the tuples merged into what one unpartitioned pass returns.  0 = automatic: one partition
        whenever the index fits the device."""
        if max_bases < 0:
            raise MuscatoError("partition bases must be >= 0")
        self._call("musc_db_set_partition_bases", int(max_bases))

    def partitions(self) -> List[int]:
        """The plan of the last build or match: partition boundaries as target numbers (n partitions, n + 1 entries;
        empty before any)."""
        n = ctypes.c_uint32()
        self._call("musc_db_partitions", None, 0, ctypes.byref(n))
        if not n.value:
            return []
        out = (ctypes.c_uint32 * (n.value + 1))()
        self._call("musc_db_partitions", out, n.value + 1, ctypes.byref(n))
        return list(out)

    def _apply_partition_bases(self, cfg: "Config") -> None:
        # (Config.DbPartitionBases > 0 is applied; 0 leaves the engine's setting: automatic, unless set_partition_bases
        # chose a limit -- call set_partition_bases(0) to return to the automatic plan)
        if cfg.DbPartitionBases:
            self.set_partition_bases(int(cfg.DbPartitionBases))

    # ---- reads (already prepared: X-substituted, truncated, unique)
    def load_reads(self, seqs: Sequence[bytes]) -> None:
        buf, off = concat(seqs)
        self.load_reads_arrays(buf, off)

    def load_reads_arrays(self, buf: np.ndarray, off: np.ndarray) -> None:
        self._call("musc_reads_load_ascii", buf.ctypes.data, off.ctypes.data, len(off) - 1, 0)
        self.n_reads = len(off) - 1

    def load_reads_device(self, seqs_ptr: int, off_ptr: int, nreads: int) -> None:
        self._call("musc_reads_load_ascii", seqs_ptr, off_ptr, nreads, 1)
        self.n_reads = nreads

    def sort_unique_reads(self, seqs: Sequence[bytes]):
        """Read prep on the GPU (musc_reads_sort_unique): `seqs` are prepared reads in input order.
        Loads the distinct sequences in bytewise order as the context's reads and returns
        (order uint32[n], ustart uint32[n_unique + 1]): distinct sequence g stands for the input
        reads order[ustart[g]:ustart[g+1]]."""
        buf, off = concat(seqs)
        return self.sort_unique_reads_arrays(buf.ctypes.data, off.ctypes.data, len(off) - 1, False)

    def sort_unique_reads_arrays(self, seqs_ptr: int, off_ptr: int, nreads: int, on_device: bool):
        po, pu, nu = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        self._call("musc_reads_sort_unique", seqs_ptr, off_ptr, nreads, 1 if on_device else 0, ctypes.byref(po), ctypes.byref(pu),
                   ctypes.byref(nu))
        order, ustart = self._take_u32((po, nreads), (pu, nu.value + 1))
        self.n_reads = int(nu.value)
        return order, ustart

    def prep_fastq(self, raw: bytes, min_len: int, max_len: int) -> dict:
        """FASTQ parsing and read prep on the GPU (musc_reads_prep_fastq): `raw` is the text of the read file.  Loads
        the distinct prepared sequences in bytewise order as the context's reads and returns the counts (n_records,
        n_short, n_reads, n_unique, max_len) and, as numpy arrays over the kept reads in file order, their spans in
        `raw` (name_off, name_len, seq_off, seq_len) and order / ustart as sort_unique_reads returns them."""
        return self._prep_fastq(False, *_host_ptr(raw), min_len, max_len, False)

    def prep_fastq_device(self, ptr: Optional[int], nbytes: int, min_len: int, max_len: int, on_device: bool = True) -> dict:
        """The same for `nbytes` of text at `ptr`: a device pointer of any alignment (the spans are offsets from it)."""
        return self._prep_fastq(False, ptr, nbytes, min_len, max_len, on_device)

    def _prep_fastq(self, names: bool, ptr: Optional[int], nbytes: int, min_len: int, max_len: int, on_device: bool) -> dict:
        """musc_reads_prep_fastq, or (names) musc_reads_prep_fastq_names, and what it filled in as the documented dict."""
        fp, info = _lib.MuscFastqPrep(), _lib.MuscReadNames()
        args = (ptr, int(nbytes), 1 if on_device else 0, int(min_len), int(max_len), ctypes.byref(fp))
        self.n_reads = 0
        if names:
            self._call("musc_reads_prep_fastq_names", *args, ctypes.byref(info))
        else:
            self._call("musc_reads_prep_fastq", *args)
        try:
            out = self._fastq_dict(fp, info if names else None)
        finally:
            self._lib.musc_fastq_prep_free(ctypes.byref(fp))
        self.n_reads = out["n_unique"]
        return out

    def _fastq_dict(self, fp: _lib.MuscFastqPrep, info: Optional[_lib.MuscReadNames]) -> dict:
        """Copies of what the structs hold: uint64 offsets; uint32 lengths, order, ustart and ranked.  Takes (frees)
        info.ranked; fp stays the caller's to free."""
        n, nu = int(fp.n_reads), int(fp.n_unique)
        ranked = self._take_u32((info.ranked, n)) if info is not None else None  # (first: it is freed whatever follows)
        out = {"n_records": int(fp.n_records), "n_short": int(fp.n_short), "n_reads": n, "n_unique": nu, "max_len": int(fp.max_len)}
        for k in ("name_off", "seq_off", "name_len", "seq_len", "order"):
            out[k] = _array(getattr(fp, k), n)
        out["ustart"] = _array(fp.ustart, nu + 1)
        if info is not None:
            out["ranked"] = ranked[0]
            out["names"] = {k: getattr(info, k) for k, _ in info._fields_ if k != "ranked"}
        return out

    # ---- the names of the reads on the device
    def names_order(self, raw: bytes, name_off, name_len, order, ustart) -> np.ndarray:
        """The members of hand-fed groups in the order of their clipped names (musc_reads_names_order): the arrays are
        those prep_fastq returns for `raw`.  -> the kept reads, group by group, ranked.  Touches no loaded reads."""
        text, nbytes = _host_ptr(raw)
        no = np.ascontiguousarray(name_off, dtype=np.uint64)
        nl = np.ascontiguousarray(name_len, dtype=np.uint32)
        od = np.ascontiguousarray(order, dtype=np.uint32)
        us = np.ascontiguousarray(ustart, dtype=np.uint32)
        n = len(od)
        if len(no) != n or len(nl) != n or len(us) < 1:
            raise MuscatoError("names_order: name_off, name_len and order must have one entry per kept read, ustart one more than the groups")
        ranked = np.zeros(max(n, 1), dtype=np.uint32)
        self._call("musc_reads_names_order", text, nbytes, 0, no.ctypes.data, nl.ctypes.data, n, od.ctypes.data, us.ctypes.data, len(us) - 1,
                   ranked.ctypes.data)
        return ranked[:n]

    def prep_fastq_names(self, raw: bytes, min_len: int, max_len: int) -> dict:
        """prep_fastq with the names ordered, cut and joined on the device (musc_reads_prep_fastq_names): the record
        ``count\\tnames`` of every distinct read is left as the context's read text, as set_read_text would leave it.
        -> the dict of prep_fastq, and "ranked" (the kept reads group by group in name order) and "names" (text_bytes,
        line_bytes, n_single, n_counted, n_sorted, n_pairs, key_passes, ms_names)."""
        return self._prep_fastq(True, *_host_ptr(raw), min_len, max_len, False)

    def prep_fastq_names_device(self, ptr: Optional[int], nbytes: int, min_len: int, max_len: int, on_device: bool = True) -> dict:
        return self._prep_fastq(True, ptr, nbytes, min_len, max_len, on_device)

    def names_text(self, which: int = 0, rec0: int = 0, nrec: Optional[int] = None) -> bytes:
        """Records [rec0, rec0 + nrec) of what prep_fastq_names rendered: which 0, the records ``count\\tnames``; which
        1, the lines ``seq\\tcount\\tnames\\n`` of reads_sorted.txt."""
        return self._text_range("musc_reads_names_text", (int(which),), rec0, nrec)

    def names_text_into(self, which: int, rec0: int, nrec: int, dst_ptr: int, capacity: int, on_device: bool) -> int:
        """The same into a buffer of the caller's, on the host or on the device -> the bytes written."""
        nb = ctypes.c_uint64()
        self._call("musc_reads_names_text", int(which), int(rec0), int(nrec), dst_ptr, int(capacity), 1 if on_device else 0,
                   ctypes.byref(nb))
        return int(nb.value)

    def load_reads_packed(self, seqs: Sequence[bytes]) -> None:
        self.n_reads = self._packed("musc_reads_load_packed", seqs)

    def load_reads_packed_ptr(self, bases_ptr: int, mask_ptr: int, off_ptr: int, nreads: int) -> None:
        """musc_reads_load_packed on caller-owned host buffers (e.g. pinned memory): 2-bit bases,
        optional 1-bit X mask (0 = none), uint64 offsets[nreads + 1] in bases."""
        self._call("musc_reads_load_packed", bases_ptr, mask_ptr or None, off_ptr, nreads)
        self.n_reads = nreads

    def load_reads_packed32_ptr(self, bases_ptr: int, mask_ptr: int, lengths_ptr: int, fixed_len: int, nreads: int,
                                async_upload: bool = False) -> None:
        """musc_reads_load_packed32: 2-bit bases back to back, optional 1-bit X mask (0 = none), uint32
        lengths (0 = every read has fixed_len bases).  async_upload (fixed length, no mask): returns
        once the upload is queued; the next match overlaps it batch by batch -- the host buffer must
        stay valid until that match returns."""
        self._call("musc_reads_load_packed32", bases_ptr, mask_ptr or None, lengths_ptr or None, fixed_len, nreads,
                   1 if async_upload else 0)
        self.n_reads = nreads

    # ---- hot path
    def match_device(self, cfg: Config, apply_mmtol: bool = True, skip_block_check: bool = False,
                     n_shards: int = 1) -> int:
        """Run screen+confirm(+select); hits stay on the device.  Returns the hit count.
        n_shards = number of read shards the (window,key) blocks are split over (world size of a
        one-process-per-GPU run): the MaxMatches proof then holds for the union of the shards."""
        p = cfg.to_params(apply_mmtol, skip_block_check, n_shards)
        self._apply_partition_bases(cfg)
        n = ctypes.c_uint64()
        self._call("musc_match_device", ctypes.byref(p), ctypes.byref(n))
        return int(n.value)

    def hits_to(self, ptr: int, capacity: int, on_device: bool) -> None:
        self._call("musc_hits_copy", ptr, capacity, 1 if on_device else 0)

    def hits_to_packed(self, ptr: int, capacity: int, on_device: bool, bits: Sequence[int], read_base: int = 0) -> None:
        """The last pass's tuples as one u64 each (read+base | gene | pos | nmiss, widths `bits`)."""
        b = (ctypes.c_int32 * 4)(*bits)
        self._call("musc_hits_copy_packed", ptr, capacity, 1 if on_device else 0, read_base, b)

    def hits_to_compact(self, words_ptr: int, words_cap: int, counts_ptr: int, counts_cap: int, on_device: bool,
                        bits: Sequence[int]) -> None:
        """The last pass's tuples as one u32 word each (gene | pos | nmiss, widths `bits`) plus one
        byte per loaded read = its number of tuples (musc_hits_copy_compact: the list is read-major)."""
        b = (ctypes.c_int32 * 3)(*bits)
        self._call("musc_hits_copy_compact", words_ptr, words_cap, counts_ptr, counts_cap, 1 if on_device else 0, b)

    def unpack_hits(self, src_ptr: int, n: int, on_device: bool, bits: Sequence[int], dst_ptr: int) -> None:
        b = (ctypes.c_int32 * 4)(*bits)
        self._call("musc_hits_unpack", src_ptr, n, 1 if on_device else 0, b, dst_ptr)

    def match(self, cfg: Config, apply_mmtol: bool = True, n_shards: int = 1) -> np.ndarray:
        """-> uint32 array [n, 4] of (read_idx, gene_idx, pos, nmiss), order unspecified."""
        n = self.match_device(cfg, apply_mmtol, n_shards=n_shards)
        out = np.zeros((n, 4), dtype=np.uint32)
        if n:
            self.hits_to(out.ctypes.data, n, False)
        return out

    def overflow_probes(self) -> np.ndarray:
        """(read_idx, window) of the probes whose (window,key) block may exceed MaxMatches after
        the last match (empty when n_overflow_blocks == 0).  uint32 [n, 2]."""
        pr, pw, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        self._call("musc_overflow_probes", ctypes.byref(pr), ctypes.byref(pw), ctypes.byref(n))
        return np.stack(self._take_u32((pr, n.value), (pw, n.value)), axis=1)

    def apply_maxmatches(self, apply_mmtol: bool = True) -> dict:
        """Replay the reference's MaxMatches truncation on the device (musc_maxmatches_apply): after a match with
        apply_mmtol=False the resident list becomes what the reference keeps (with apply_mmtol=True: of that, per read,
        nmiss <= best + MMTol).  hits_to*, results_order() and the side stage read the new list.
        -> {"nhits", "suspect_probes", "truncated_blocks"}.  MuscatoError "(2)": no such pass; "(12)": a shape the
        device stage does not take (the context is untouched)."""
        n, ns, nt = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._call("musc_maxmatches_apply", 1 if apply_mmtol else 0, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(nt))
        return {"nhits": int(n.value), "suspect_probes": int(ns.value), "truncated_blocks": int(nt.value)}

    def maxmatches_ms(self) -> float:
        """HIP-event time of the last apply_maxmatches."""
        ms = ctypes.c_float()
        self._call("musc_maxmatches_last_ms", ctypes.byref(ms))
        return float(ms.value)

    def maxmatches_detail(self) -> dict:
        """Of the last apply_maxmatches: the pairs its truncated blocks held, and the time of k_mm_replay alone."""
        n, ms = ctypes.c_uint64(), ctypes.c_float()
        self._call("musc_maxmatches_last_detail", ctypes.byref(n), ctypes.byref(ms))
        return {"pairs": int(n.value), "replay_ms": float(ms.value)}

    def hits(self) -> np.ndarray:
        """The resident list (of the last match, or of apply_maxmatches) -> uint32 [n, 4]."""
        n = int(self.stats()["n_hits"])
        out = np.zeros((n, 4), dtype=np.uint32)
        if n:
            self.hits_to(out.ctypes.data, n, False)
        return out

    def last_instance(self) -> dict:
        """The kernel instances the last match launched, from the resolver that returned their function pointers:
        {"path": "fused" | "two-kernel" | "none", "match": k_match_t / k_match_g descriptor or None, "screen": k_screen /
        k_screen_t descriptor or None, "confirm": k_confirm descriptor or None, "block_mode": 0 | 1 | 2, "exact_rerun":
        the pass repeated one whose MaxMatches screening was inconclusive}; a descriptor is decode_instance's dict."""
        w = (ctypes.c_uint32 * _INSTANCE_WORDS)()
        self._call("musc_last_instance", w)
        return {"path": "fused" if w[0] else "two-kernel" if w[1] else "none",
                "match": decode_instance(w[0]), "screen": decode_instance(w[1]), "confirm": decode_instance(w[2]),
                "block_mode": w[3] & 0xFF, "exact_rerun": bool(w[3] & 0x100)}

    # ---- results.txt from the resident tuples (cmd/muscato/main.go:422-676 on the device)
    def set_gene_text(self, id_rests: Sequence[bytes], absent: Optional[Sequence[bool]] = None) -> None:
        """Gene g's ``name\\tlen`` (what follows the gene number on its id line); absent[g] true = the id file has no
        line for gene g: its tuples vanish from the results.  Forgotten by the next target load.
        The device renders and orders targetsub from the packed targets (2 bits a base + an X plane): every target
        byte that is none of A C G T comes out as ``X`` in the lines."""
        buf, off = concat(list(id_rests))
        ab = None
        if absent is not None:
            ab = np.ascontiguousarray(np.asarray(absent, dtype=bool).astype(np.uint8))
            if len(ab) != len(id_rests):
                raise MuscatoError("absent must have one entry per gene")
        self._call("musc_results_set_gene_text", buf.ctypes.data, off.ctypes.data, ab.ctypes.data if ab is not None else None,
                   len(off) - 1)

    def set_read_text(self, tails: Sequence[bytes]) -> None:
        """Read r's ``count\\tnames`` tail.  Without it a line ends after its sixth column.  Forgotten by the next
        read load."""
        buf, off = concat(list(tails))
        self._call("musc_results_set_read_text", buf.ctypes.data, off.ctypes.data, len(off) - 1)

    def results_order(self, hits: Optional[np.ndarray] = None) -> Tuple[int, int]:
        """Order tuples as the lines of results.txt are ordered and compute the line offsets -> (nlines, nbytes).
        hits: uint32 [n, 4] of (read_idx, gene_idx, pos, nmiss) in any order, or None = the list the last match left
        on the device.  Tuples of absent genes are dropped."""
        nl, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._res_nlines = 0
        ptr, n = None, 0
        if hits is not None:
            # (a NULL list means "the device list": an empty host list still passes a pointer)
            a = np.ascontiguousarray(np.asarray(hits, dtype=np.uint32).reshape(-1, 4))
            pad = np.zeros((1, 4), dtype=np.uint32)
            ptr, n = (a.ctypes.data if len(a) else pad.ctypes.data), len(a)
        self._call("musc_results_order", ptr, n, 0, ctypes.byref(nl), ctypes.byref(nb))
        self._res_nlines = int(nl.value)
        return int(nl.value), int(nb.value)

    def results_hits(self) -> np.ndarray:
        """The tuples of the last results_order, in line order: uint32 [nlines, 4]."""
        out = np.zeros((self._res_nlines, 4), dtype=np.uint32)
        self._call("musc_results_hits", out.ctypes.data, self._res_nlines, 0)
        return out

    def _text_range(self, name: str, head: tuple, rec0: int, nrec: Optional[int]) -> bytes:
        """Records [rec0, rec0 + nrec) of the text call `name(ctx, *head, rec0, nrec, dst, capacity, on_device, &nbytes)`;
        an empty range is b"" after the sizing call alone."""
        count = (1 << 62) if nrec is None else int(nrec)
        return self._sized(lambda dst, cap, nb: self._call(name, *head, int(rec0), count, dst, cap, 0, nb), skip_empty=True)

    def results_text(self, line0: int = 0, nlines: Optional[int] = None) -> bytes:
        """The bytes of lines [line0, line0 + nlines) of the last results_order (nlines None: to the end); the
        concatenation over consecutive ranges is results.txt."""
        return self._text_range("musc_results_text", (), line0, nlines)

    def results_ms(self) -> Tuple[float, float]:
        """HIP-event milliseconds of the last results_order and of the results_text calls since."""
        return self._ms_pair("musc_results_last_ms")

    # ---- the side outputs of a pass from the resident tuples
    def side_prepare(self) -> dict:
        """Build the nonmatch FASTQ, genestats and readstats of the last results_order on the device ->
        {"nonmatch": (nrecords, nbytes), "genestats": ..., "readstats": ...}.  Needs the read text, and a gene text
        whose entries are all ``name\\tlen`` without blanks (MuscatoError with code 12 otherwise)."""
        nr, nb = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
        self._call("musc_side_prepare", nr, nb)
        return {k: (int(nr[w]), int(nb[w])) for w, k in enumerate(("nonmatch", "genestats", "readstats"))}

    def _side_text(self, which: int, rec0: int, nrec: Optional[int]) -> bytes:
        return self._text_range("musc_side_text", (which,), rec0, nrec)

    def nonmatch_text(self, rec0: int = 0, nrec: Optional[int] = None) -> bytes:
        """FASTQ records [rec0, rec0 + nrec) of the reads without a results line (nrec None: to the end)."""
        return self._side_text(_lib.SIDE_NONMATCH, rec0, nrec)

    def genestats_text(self, rec0: int = 0, nrec: Optional[int] = None) -> bytes:
        """Lines [rec0, rec0 + nrec) of ``name\\tN\\t``: the kept tuples per gene name, in name order."""
        return self._side_text(_lib.SIDE_GENESTATS, rec0, nrec)

    def readstats_text(self, rec0: int = 0, nrec: Optional[int] = None) -> bytes:
        """Lines [rec0, rec0 + nrec) of ``token\\tname;name;``: per run of matched reads with one first name, its genes."""
        return self._side_text(_lib.SIDE_READSTATS, rec0, nrec)

    def side_ms(self) -> Tuple[float, float]:
        """HIP-event milliseconds of the last side_prepare and of the text calls since."""
        return self._ms_pair("musc_side_last_ms")

    # ---- SAM output from the resident tuples
    def sam_prepare(self, rev_pairs: bool = False) -> dict:
        """Compare every span of the last results_order with its read and lay out the SAM records and the header ->
        {"records": n, "header_bytes": b, "record_bytes": b}.  rev_pairs: the database holds reverse complements, target
        2k + 1 that of target 2k.  MuscatoError with code 12: rev_pairs with an odd number of targets or a pair of
        unequal lengths, or a gene text whose first token is empty."""
        _sam.bind()
        n, hb, rb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._call("musc_sam_prepare", 1 if rev_pairs else 0, ctypes.byref(n), ctypes.byref(hb), ctypes.byref(rb))
        return {"records": int(n.value), "header_bytes": int(hb.value), "record_bytes": int(rb.value)}

    def sam_header(self) -> bytes:
        """The header of the last sam_prepare: @HD, one @SQ per target with an id line, @PG."""
        _sam.bind()
        return self._text_range("musc_sam_text", (_sam.SAM_HEADER,), 0, None)

    def sam_text(self, rec0: int = 0, nrec: Optional[int] = None) -> bytes:
        """Records [rec0, rec0 + nrec) of the last sam_prepare (nrec None: to the end), one per line of results.txt in
        the same order; header + the concatenation over consecutive ranges is the SAM file."""
        _sam.bind()
        return self._text_range("musc_sam_text", (_sam.SAM_RECORDS,), rec0, nrec)

    def sam_text_into(self, which: int, rec0: int, nrec: int, dst_ptr: int, capacity: int, on_device: bool) -> int:
        """Records [rec0, rec0 + nrec) of text `which` (0 header, 1 records) into caller memory (host or device) ->
        the bytes written."""
        _sam.bind()
        nb = ctypes.c_uint64()
        self._call("musc_sam_text", int(which), int(rec0), int(nrec), dst_ptr, int(capacity), 1 if on_device else 0, ctypes.byref(nb))
        return int(nb.value)

    def sam_ms(self) -> Tuple[float, float]:
        """HIP-event milliseconds of the last sam_prepare and of the text calls since."""
        _sam.bind()
        return self._ms_pair("musc_sam_last_ms")

    # ---- coverage from the resident tuples
    def cov_prepare(self, rev_pairs: bool = False, weighted: bool = False, unique: bool = False) -> dict:
        """Sort the interval ends of the last results_order, sum them to depths and lay out the bedGraph and the summary
        -> {"runs": n, "run_bytes": b, "targets": n, "summary_bytes": b}.  rev_pairs: target 2k + 1 is the reverse strand
        of target 2k; weighted: a line counts by its read's count; unique: only the lines of reads with one line count.
        MuscatoError with code 12: a total weight of 2^32 or more, 2^31 lines or more, rev_pairs with an odd number of
        targets or a pair of unequal lengths, or a gene text whose first token is empty."""
        _cov.bind()
        flags = (_cov.COV_REV_PAIRS if rev_pairs else 0) | (_cov.COV_WEIGHTED if weighted else 0) | (_cov.COV_UNIQUE if unique else 0)
        n, rb, nt, sb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._call("musc_cov_prepare", flags, ctypes.byref(n), ctypes.byref(rb), ctypes.byref(nt), ctypes.byref(sb))
        return {"runs": int(n.value), "run_bytes": int(rb.value), "targets": int(nt.value), "summary_bytes": int(sb.value)}

    def cov_bedgraph(self, rec0: int = 0, nrec: Optional[int] = None) -> bytes:
        """Records [rec0, rec0 + nrec) of the bedGraph of the last cov_prepare (nrec None: to the end): one per run of
        constant non-zero depth, `rname start end depth`, in target order."""
        _cov.bind()
        return self._text_range("musc_cov_text", (_cov.COV_BEDGRAPH,), rec0, nrec)

    def cov_summary(self, rec0: int = 0, nrec: Optional[int] = None) -> bytes:
        """Records [rec0, rec0 + nrec) of the summary of the last cov_prepare: one per target with an id line,
        `rname len numreads covbases sumdepth maxdepth`."""
        _cov.bind()
        return self._text_range("musc_cov_text", (_cov.COV_SUMMARY,), rec0, nrec)

    def cov_text_into(self, which: int, rec0: int, nrec: int, dst_ptr: int, capacity: int, on_device: bool) -> int:
        """Records [rec0, rec0 + nrec) of text `which` (0 bedGraph, 1 summary) into caller memory (host or device) ->
        the bytes written."""
        _cov.bind()
        nb = ctypes.c_uint64()
        self._call("musc_cov_text", int(which), int(rec0), int(nrec), dst_ptr, int(capacity), 1 if on_device else 0, ctypes.byref(nb))
        return int(nb.value)

    def cov_ms(self) -> Tuple[float, float]:
        """HIP-event milliseconds of the last cov_prepare and of the text calls since."""
        _cov.bind()
        return self._ms_pair("musc_cov_last_ms")

    def stats(self) -> dict:
        s = _lib.MuscStats()
        self._call("musc_get_stats", ctypes.byref(s))
        return {k: getattr(s, k) for k, _ in s._fields_}


_INSTANCE_WORDS = 4  # MUSC_INSTANCE_WORDS
# family (MUSC_INST_*) -> the kernel and its template arguments after RW, in descriptor order
_INST_FIELDS = {1: ("k_match_t", ("W", "XM", "WIDE", "SG")), 2: ("k_match_g", (None, None, None, "SG")),
                3: ("k_screen", ("mask", "one", "lines")), 4: ("k_screen_t", ()), 5: ("k_confirm", ("mask", "w2"))}


def number_key(pos: int, nmiss: int) -> int:
    """``pos \\t nmiss`` of a results line as one integer that compares as that text does bytewise (no GPU needed):
    4 bits a decimal digit (digit + 1), left-aligned, ten digits of pos above five of nmiss."""
    k = ctypes.c_uint64()
    if _lib.load().musc_results_number_key(int(pos), int(nmiss), ctypes.byref(k)):
        raise ValueError("number_key: nmiss %d has more than five digits" % nmiss)
    return int(k.value)


def decode_instance(word: int) -> Optional[dict]:
    """A descriptor word of musc_last_instance / musc_instances (include/muscato_hip.h) as
    {"kernel": name, "RW": .., <template argument>: ..}; None for 0 (no such kernel in the pass)."""
    if not word:
        return None
    name, fields = _INST_FIELDS[word & 0xFF]
    d = {"kernel": name, "RW": (word >> 8) & 0xFF}
    for i, f in enumerate(fields):
        if f:
            d[f] = (word >> (16 + 4 * i)) & 0xF
    return d


def instance_name(d: Optional[dict]) -> str:
    """k_match_t<8, 2, 0, 0, 0> for a decoded descriptor, in the template's argument order."""
    return "none" if d is None else "%s<%s>" % (d["kernel"], ", ".join(str(v) for k, v in d.items() if k != "kernel"))


def instances() -> List[dict]:
    """Every kernel instance the library's resolvers can return (no GPU needed)."""
    lib = _lib.load()
    n = ctypes.c_uint32()
    if lib.musc_instances(None, 0, ctypes.byref(n)):
        raise RuntimeError("musc_instances failed")
    buf = (ctypes.c_uint32 * max(1, n.value))()
    lib.musc_instances(buf, n.value, ctypes.byref(n))
    return [decode_instance(w) for w in buf[:n.value]]


def stream_plan(nreads: int, fixed_len: int, batch_reads: int = 16 << 20) -> dict:
    """The schedule of a streamed load of `nreads` reads of `fixed_len` bases (no GPU needed): {"piece_ends": read
    index each piece of the upload ends before, "batch_ends": where the batches of the pass that consumes it end (a
    subset of piece_ends), "planned_batches": the batch count the MaxMatches screening threshold is divided by}."""
    lib = _lib.load()
    n, planned = ctypes.c_uint64(), ctypes.c_uint64()
    if lib.musc_stream_plan(nreads, fixed_len, batch_reads, None, None, 0, ctypes.byref(n), ctypes.byref(planned)):
        raise ValueError("musc_stream_plan: %d reads of %d bases is not a read set the loader takes" % (nreads, fixed_len))
    ends = np.zeros(max(1, n.value), dtype=np.uint64)
    flags = np.zeros(max(1, n.value), dtype=np.uint8)
    lib.musc_stream_plan(nreads, fixed_len, batch_reads, ends.ctypes.data, flags.ctypes.data, n.value, ctypes.byref(n),
                         ctypes.byref(planned))
    ends, flags = ends[:n.value], flags[:n.value]
    return {"piece_ends": ends, "batch_ends": ends[flags != 0], "planned_batches": int(planned.value)}


def gather(engines: Sequence["Engine"], read_bases: Sequence[int], rccl: bool = False) -> np.ndarray:
    """Concatenate the device-resident hits of several engines of ONE process in order, adding
    read_bases[i] to the read_idx of engine i (musc_gather: every GPU copies its own to the host;
    rccl=True, opt-in: musc_gather_rccl, over RCCL/xGMI to the first engine's GPU and one copy to the
    host -- any failure there falls back to musc_gather).  uint32 [n, 4]."""
    lib = engines[0]._lib
    n = len(engines)
    arr = (ctypes.c_void_p * n)(*[e._h for e in engines])
    bases = (ctypes.c_uint64 * n)(*[int(b) for b in read_bases])
    ph, cnt = ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib.musc_gather_rccl(arr, n, bases, ctypes.byref(ph), ctypes.byref(cnt)) if rccl else 1
    if rccl and rc == 2:  # a caller's mistake (contexts sharing a device, ...): not something to paper over
        raise MuscatoError("musc_gather_rccl failed (%d): %s" % (rc, lib.musc_last_error(engines[0]._h).decode()))
    if rc != 0:
        rc = lib.musc_gather(arr, n, bases, ctypes.byref(ph), ctypes.byref(cnt))
    if rc != 0:
        raise MuscatoError("musc_gather failed (%d): %s" % (rc, lib.musc_last_error(engines[0]._h).decode()))
    out = np.zeros((cnt.value, 4), dtype=np.uint32)
    if cnt.value:
        ctypes.memmove(out.ctypes.data, ph, cnt.value * 16)
    lib.musc_free_hits(ph)
    return out


def sorted_hits(a: np.ndarray) -> np.ndarray:
    """Canonical order (read, gene, pos, nmiss) for comparisons."""
    if len(a) == 0:
        return a.reshape(0, 4)
    idx = np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))
    return a[idx]
