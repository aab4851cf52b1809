"""Packed members on the device (include/skyrim_pack.h): the listed channels of M member states as 16-bit codes in a
netCDF-3 file's byte order, and the way back.

Layers:

* the binding of libskyrim_pack.so (``SPEC``, ``load_library``, ``run_range``, ``run_quantize``, ``run_unpack``); the same calls are
  ``torch.ops.skyrim_hip.pack_range``, ``pack_quantize`` and ``pack_unpack``.  None has a CPU fallback;
* ``ENTRY``, the numpy dtype of a table record (``skpack_entry``), and ``table_of`` / ``new_table``, which carry a table between a device
  tensor and the host;
* ``pack_members``: range and codes of M states in two calls, the image and the table left on the device; ``packed_dataarray``: one
  member's image as a packed DataArray, which ncio.py writes with the image handed to ``pwrite`` untouched;
* ``check_request`` and ``LeadArchive``: ``ensemble_forecast(archive={...})``, a stage of the ensemble driver that writes one file per
  (member, saved lead) and a ``manifest.json``;
* ``open`` -> ``MemberArchive`` (``info``, ``member``, ``states``, ``replay``) and ``ArchiveMembers``, the member source that lets the
  driver run its stage list on a forecast that was written down, without a model and without weights.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np

from . import native
from .members import member_set

# include/skyrim_pack.h SKPACK_*
MAX_MEMBERS, MAX_CHANNELS, RANGE_TILE, FILL = 1024, 256, 16384, -32768
_P = ctypes.c_void_p
ENTRY = np.dtype([("offset", "<f8"), ("scale", "<f8"), ("inv", "<f8"), ("lo", "<f4"), ("hi", "<f4"), ("n_bad", "<i4"), ("pad", "<i4")])


class Entry(ctypes.Structure):
    """skpack_entry."""
    _fields_ = [("offset", ctypes.c_double), ("scale", ctypes.c_double), ("inv", ctypes.c_double), ("lo", ctypes.c_float),
                ("hi", ctypes.c_float), ("n_bad", ctypes.c_int32), ("pad", ctypes.c_int32)]


class Desc(ctypes.Structure):
    """skpack_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("nc", ctypes.c_int),
                ("channels", ctypes.c_int32 * MAX_CHANNELS), ("table", _P), ("workspace", _P), ("workspace_bytes", ctypes.c_size_t),
                ("out", _P), ("member_stride_bytes", ctypes.c_size_t)]


class UnpackDesc(ctypes.Structure):
    """skpack_unpack_desc."""
    _fields_ = [("codes", _P), ("table", _P), ("nc", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("out", _P)]


SPEC = native.Spec("skyrim_pack", "SKYRIM_PACK_LIB", "skpack", 1, {              # include/skyrim_pack.h SKPACK_ABI_VERSION
    "skpack_abi_version": (ctypes.c_int, []),
    "skpack_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "skpack_range": (ctypes.c_int, [ctypes.POINTER(Desc), _P]),
    "skpack_quantize": (ctypes.c_int, [ctypes.POINTER(Desc), _P]),
    "skpack_unpack": (ctypes.c_int, [ctypes.POINTER(UnpackDesc), _P]),
    "skpack_range_check": (ctypes.c_int, [ctypes.POINTER(Desc)]),
    "skpack_quantize_check": (ctypes.c_int, [ctypes.POINTER(Desc)]),
    "skpack_unpack_check": (ctypes.c_int, [ctypes.POINTER(UnpackDesc)]),
}, " -- packed member archives have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_pack.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def describe(M, C, H, W, channels) -> Desc:
    """The descriptor of ``skpack_range`` / ``skpack_quantize``, its pointers still NULL."""
    d = Desc()
    d.M, d.C, d.H, d.W = int(M), int(C), int(H), int(W)
    channels = [int(c) for c in channels]
    d.nc = len(channels)
    for k, c in enumerate(channels[:MAX_CHANNELS]):
        d.channels[k] = c
    return d


def workspace_bytes(M, nc, H, W) -> int:
    """Bytes of workspace ``pack_range`` needs (0 for counts outside their ranges)."""
    return int(load_library().skpack_workspace_bytes(int(M), int(nc), int(H), int(W)))


def new_table(M, nc, device):
    """An uninitialised (M, nc) table on ``device``: a float64 tensor (M, nc, 5), five doubles being the 40 bytes of a record."""
    import torch
    return torch.empty((int(M), int(nc), ENTRY.itemsize // 8), dtype=torch.float64, device=device)


def table_of(t) -> np.ndarray:
    """The records of a table tensor (device or host) as a numpy array of dtype ``ENTRY``, shaped like its leading dimensions."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(ENTRY).reshape(a.shape[:-1])


def table_tensor(records, device):
    """The table tensor (``new_table``'s layout) of host records of dtype ``ENTRY``."""
    import torch
    r = np.ascontiguousarray(records, ENTRY)
    return torch.from_numpy(r.view(np.float64).reshape(r.shape + (ENTRY.itemsize // 8,)).copy()).to(device)


def _table_ptr(table, what, n, dev) -> int:
    import torch
    p = native.tensor_ptr(table, f"{what}: table", torch.float64, dev)
    if table.numel() != n * (ENTRY.itemsize // 8):
        raise ValueError(f"{what}: table must hold {n} records of {ENTRY.itemsize} bytes (archive.new_table)")
    return p


def _common(what, members, table, channels, tab):
    channels = [int(c) for c in channels]
    M, dev, _ = member_set(members, table, what, MAX_MEMBERS)
    C, H, W = members[0].shape
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"{what}: {len(channels)} channels; 1 to {MAX_CHANNELS} per call (SKPACK_MAX_CHANNELS)")
    if any(not 0 <= c < C for c in channels):
        raise ValueError(f"{what}: a channel index lies outside 0..{C - 1}")
    if C * H * W > 2 ** 30 or len(channels) * H * W > 2 ** 30:
        raise ValueError(f"{what}: a state holds at most 2^30 elements, and so do the listed planes of a call")
    d = describe(M, C, H, W, channels)
    d.members, d.table = table.data_ptr(), _table_ptr(tab, what, M * len(channels), dev)
    return d, dev


def run_range(members, table, channels, tab, workspace) -> None:
    """One ``skpack_range``: the records of the listed ``channels`` of the M ``members`` (equal-shaped contiguous float32 (C, H, W) device
    tensors; ``table`` = ``member_table(members)``) into ``tab`` (``new_table(M, nc, device)``).  ``workspace``: a uint8 device tensor of
    ``workspace_bytes(M, nc, H, W)`` at least.  Queued on torch's current stream."""
    import torch
    what = "pack_range"
    d, dev = _common(what, members, table, channels, tab)
    d.workspace = native.tensor_ptr(workspace, f"{what}: workspace", torch.uint8, dev)
    d.workspace_bytes = workspace.numel()
    if d.workspace_bytes < workspace_bytes(d.M, d.nc, d.H, d.W) or d.workspace % 4:
        raise ValueError(f"{what}: workspace must hold {workspace_bytes(d.M, d.nc, d.H, d.W)} bytes, 4-byte aligned")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skpack_range(ctypes.byref(d), native.stream(dev)), "skpack_range", lib)


def run_quantize(members, table, channels, tab, out, member_stride_bytes=None) -> None:
    """One ``skpack_quantize``: the big-endian codes of the listed channels of member m into the uint8 device tensor ``out`` from byte
    ``m * member_stride_bytes`` (default: 2 nc H W, the members back to back); ``out`` may be a view at any even address."""
    import torch
    what = "pack_quantize"
    d, dev = _common(what, members, table, channels, tab)
    need = 2 * d.nc * d.H * d.W
    stride = need if member_stride_bytes is None else int(member_stride_bytes)
    d.out = native.tensor_ptr(out, f"{what}: out", torch.uint8, dev)
    if stride % 2 or stride < need or d.out % 2:
        raise ValueError(f"{what}: member_stride_bytes must be even and at least {need}, out 2-byte aligned")
    if out.numel() < (d.M - 1) * stride + need:
        raise ValueError(f"{what}: out holds {out.numel()} bytes, the {d.M} images end at byte {(d.M - 1) * stride + need}")
    d.member_stride_bytes = stride
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skpack_quantize(ctypes.byref(d), native.stream(dev)), "skpack_quantize", lib)


def run_unpack(codes, tab, out) -> None:
    """One ``skpack_unpack``: ``codes``, a uint8 device tensor holding the big-endian image of (nc, H, W) codes (a view at any even
    address), with the nc records ``tab`` into ``out``, float32 (nc, H, W)."""
    import torch
    what = "pack_unpack"
    if not isinstance(out, torch.Tensor) or out.dim() != 3:
        raise ValueError(f"{what}: out is (nc, H, W)")
    dev = out.device
    nc, H, W = out.shape
    d = UnpackDesc()
    d.out = native.tensor_ptr(out, f"{what}: out", torch.float32, dev)
    d.codes = native.tensor_ptr(codes, f"{what}: codes", torch.uint8, dev)
    d.table = _table_ptr(tab, what, nc, dev)
    if not 1 <= nc <= MAX_CHANNELS or nc * H * W > 2 ** 30:
        raise ValueError(f"{what}: 1 to {MAX_CHANNELS} planes of at most 2^30 elements together")
    if codes.numel() != 2 * nc * H * W or d.codes % 2:
        raise ValueError(f"{what}: codes must hold the {2 * nc * H * W} bytes of ({nc}, {H}, {W}) codes, 2-byte aligned")
    d.nc, d.H, d.W = nc, H, W
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skpack_unpack(ctypes.byref(d), native.stream(dev)), "skpack_unpack", lib)


# ---- members to images, images to files -------------------------------------------------------------------------------------------------- #
def pack_members(members, channels, table=None):
    """(image, tab) of the M ``members``: ``image`` a uint8 device tensor (M, 2 nc H W) of big-endian codes, ``tab`` the (M, nc) table,
    both still on the device and queued on the current stream: one ``pack_range`` and one ``pack_quantize``, nothing read back between."""
    import torch
    from .members import member_table
    table = member_table(members) if table is None else table
    M, (C, H, W), nc, dev = len(members), members[0].shape, len(channels), members[0].device
    tab = new_table(M, nc, dev)
    ws = torch.empty(max(workspace_bytes(M, nc, H, W), 4), dtype=torch.uint8, device=dev)
    image = torch.empty((M, 2 * nc * H * W), dtype=torch.uint8, device=dev)
    run_range(members, table, channels, tab, ws)
    run_quantize(members, table, channels, tab, image)
    return image, tab


def packed_dataarray(image, records, time, names, lat, lon, name=None):
    """One state (one time entry) as a packed ``DataArray``: ``image`` the 2 nc H W big-endian bytes (a uint8 array, e.g. over pinned
    memory), ``records`` its nc table records.  ``write_dataarray_netcdf3`` writes it with the image as the payload."""
    from .labeled import DataArray
    from .ncio import PackedImage
    records = np.asarray(records, ENTRY).reshape(1, len(names))
    img = PackedImage(image, (1, len(names), len(lat), len(lon)), records["scale"], records["offset"])
    return DataArray(img.values, ["time", "channel", "lat", "lon"],
                     dict(time=np.asarray([np.datetime64(time, "ns")]), channel=np.asarray(list(names)), lat=np.asarray(lat), lon=np.asarray(lon)),
                     name, packed=img)


# ---- the request ------------------------------------------------------------------------------------------------------------------------- #
PACKINGS = ("int16", "float32")
RING = 4                                                   # pinned slots between the copy stream and the save threads
WRITERS = 4                                                # save threads: files written side by side (ncio.py has the measurement)
MANIFEST = "manifest.json"


def check_request(names, request, save) -> dict:
    """The checked ``archive=`` request of ``ensemble_forecast``: ``{"packing": "int16" | "float32", "channels": [...] | None, "dir":
    None}``.  Refused before anything touches the device: a request that is no dict, an unknown key or packing, unknown or repeated
    channels, and a request with nowhere to write (neither ``save=True`` nor a ``"dir"``)."""
    if not isinstance(request, dict):
        raise ValueError('archive= is a dict: {"packing": "int16" | "float32", "channels": [...] | None, "dir": None}')
    unknown = [k for k in request if k not in ("packing", "channels", "dir")]
    if unknown:
        raise ValueError(f"archive: unknown keys {unknown}; it takes packing, channels and dir")
    packing = request.get("packing", "int16")
    if packing not in PACKINGS:
        raise ValueError(f"archive: packing = {packing!r}; choose from {PACKINGS}")
    channels = request.get("channels")
    channels = list(names) if channels is None else [str(c) for c in channels]
    missing = [c for c in channels if c not in names]
    if missing or not channels or len(set(channels)) != len(channels):
        raise ValueError(f"archive: channels {missing or channels} -- distinct output channels of this model, at least one")
    if len(channels) > MAX_CHANNELS:
        raise ValueError(f"archive: {len(channels)} channels; at most {MAX_CHANNELS} (SKPACK_MAX_CHANNELS)")
    if not save and not request.get("dir"):
        raise ValueError('archive= writes files: it needs save=True (under <output_dir>/<forecast_id>/members/) or a "dir"')
    return dict(packing=packing, channels=channels, indices=[list(names).index(c) for c in channels], dir=request.get("dir"))


def member_file(model_name, M, m, source, start, valid) -> str:
    """``{model}-ens{M}-m{mmm}__{src}__{start}__{valid}.nc``: the layout of every other file of a forecast."""
    from .common import generate_filename
    return generate_filename(f"{model_name}-ens{M}-m{m:03d}", start, valid, source)


# ---- writing: a stage of the ensemble driver ---------------------------------------------------------------------------------------------- #
class _Slot:
    """A pinned image and a pinned table: what one member's file is written from."""

    def __init__(self, nbytes, nc):
        import torch
        self.image = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.tab = torch.empty((nc, ENTRY.itemsize // 8), dtype=torch.float64).pin_memory()
        self.done = None


class LeadArchive:
    """The archive stage of ``ensemble.stages`` (due at saved leads, right after the raw products, so a non-finite member has already
    raised).  Per lead: ONE ``pack_range`` and ONE ``pack_quantize`` over all members into a device image allocated once (``float32``: one
    ``skio_bswap32`` per member and run of consecutive channels, no table); then per member an asynchronous copy of its image and table on
    a copy stream into one of ``RING`` pinned slots, and a save thread that writes the file from the slot: header and table through ncio,
    the payload the pinned bytes untouched.  The driver thread waits only when every slot is still being written.  ``finish`` waits for
    the files, writes ``manifest.json`` and hangs the ``MemberArchive`` on the forecast; ``close`` ends the threads, also after an error,
    and leaves no ``.part`` file behind."""

    def __init__(self, gm, p, start_time):
        model = gm.model
        self.req, self.M, self.start, self.model_name, self.source = p.archive, p.M, start_time, gm.model_name, gm.source_label
        self.names, self.indices = self.req["channels"], self.req["indices"]
        self.lat, self.lon, self.dev = np.asarray(model.grid.lat), np.asarray(model.grid.lon), model.device
        self.step = model.time_step
        self.meta = dict(model=gm.model_name, n_members=p.M, seed=int(p.asked.seed), perturbation=p.noise.kind,
                         perturb_scale=None if p.asked.perturb_scale is None else float(p.asked.perturb_scale))
        self.dir = None if self.req["dir"] is None else self._made(self.req["dir"])
        self.leads, self.files, self.n_bad = [], [], []
        self.image = None
        self.pool = self.free = self.copy = self.copied = None
        self.jobs = []

    @staticmethod
    def _made(d):
        d = Path(d)
        d.mkdir(parents=True, exist_ok=True)
        return d

    def _setup(self, L):
        import queue
        from concurrent.futures import ThreadPoolExecutor
        import torch
        if self.dir is None:
            from .common import OUTPUT_DIR
            self.dir = self._made(Path(L.sink[0].get("output_dir") or OUTPUT_DIR) / L.sink[0]["forecast_id"] / "members")
        nc, hw = len(self.indices), self.lat.size * self.lon.size
        self.width = 2 if self.req["packing"] == "int16" else 4
        self.nbytes = self.width * nc * hw
        self.image = torch.empty((self.M, self.nbytes), dtype=torch.uint8, device=self.dev)
        if self.width == 2:
            self.tab = new_table(self.M, nc, self.dev)
            self.ws = torch.empty(max(workspace_bytes(self.M, nc, self.lat.size, self.lon.size), 4), dtype=torch.uint8, device=self.dev)
        else:                                              # runs of consecutive channels: one swap each
            self.runs, i = [], 0
            while i < nc:
                j = i
                while j + 1 < nc and self.indices[j + 1] == self.indices[j] + 1:
                    j += 1
                self.runs.append((i, self.indices[i], j - i + 1))
                i = j + 1
        self.free = queue.Queue()
        for _ in range(min(RING, self.M)):
            self.free.put(_Slot(self.nbytes, nc))
        self.copy = torch.cuda.Stream(self.dev)
        self.pool = ThreadPoolExecutor(max_workers=min(WRITERS, self.M), thread_name_prefix="skyrim-archive")

    def add(self, L) -> None:
        import torch
        from . import deliver
        if self.image is None:
            self._setup(L)
        main = torch.cuda.current_stream(self.dev)
        if self.copied is not None:
            main.wait_event(self.copied)                   # the copies of the lead before read the image this lead overwrites
        nc, hw = len(self.indices), self.lat.size * self.lon.size
        if self.width == 2:
            run_range(L.states, L.table, self.indices, self.tab, self.ws)
            run_quantize(L.states, L.table, self.indices, self.tab, self.image)
        else:
            for m, st in enumerate(L.states):
                img = self.image[m].view(torch.int32)
                for at, c0, n in self.runs:
                    deliver.bswap32(st[c0:c0 + n], img[at * hw:(at + n) * hw], main)
        packed = torch.cuda.Event()
        packed.record(main)
        self.copy.wait_event(packed)
        names, bad = [], [None] * self.M
        for m in range(self.M):
            slot = self.free.get()                         # blocks only while every slot is still being written
            self._raise_failed()
            with torch.cuda.stream(self.copy):
                slot.image.copy_(self.image[m], non_blocking=True)
                if self.width == 2:
                    slot.tab.copy_(self.tab[m], non_blocking=True)
                slot.done = torch.cuda.Event()
                slot.done.record(self.copy)
            name = member_file(self.model_name, self.M, m, self.source, self.start, L.time)
            names.append(name)
            self.jobs.append(self.pool.submit(self._write, slot, m, L.time, name, bad))
        self.copied = torch.cuda.Event()
        self.copied.record(self.copy)
        self.leads.append((int(L.k), L.time))
        self.files.append(names)
        self.n_bad.append(bad)

    def _raise_failed(self):
        for j in self.jobs:
            if j.done() and not j.cancelled() and j.exception() is not None:
                raise j.exception()

    def _write(self, slot, m, time, name, bad):
        """A save thread: the file of member ``m`` at ``time`` from ``slot``, which goes back to the ring whatever happens."""
        from .ncio import write_dataarray_netcdf3
        try:
            slot.done.synchronize()
            nc, H, W = len(self.names), self.lat.size, self.lon.size
            image = slot.image.numpy()
            if self.width == 2:
                rec = table_of(slot.tab)
                bad[m] = [int(v) for v in rec["n_bad"]]
                da = packed_dataarray(image, rec, time, self.names, self.lat, self.lon)
            else:
                from .deliver import BigEndianImage
                from .labeled import DataArray
                native_ = np.empty((1, nc, H, W), np.float32)      # never filled, never read: the writer takes the image
                da = DataArray(native_, ["time", "channel", "lat", "lon"],
                               dict(time=np.asarray([np.datetime64(time, "ns")]), channel=np.asarray(self.names), lat=self.lat, lon=self.lon),
                               image=BigEndianImage(image.view(">f4").reshape(1, nc, H, W), native_))
            write_dataarray_netcdf3(da, self.dir / name, fast_threshold=0)
        finally:
            self.free.put(slot)

    def finish(self, ens) -> None:
        """(After ``close``: every file is closed.)  A save thread's error raised, else the manifest written, the ``MemberArchive`` on
        ``ens.archive`` and its files in ``ens.paths``."""
        import json
        from .common import iso
        self.close()
        for j in self.jobs:
            j.result()
        manifest = dict(self.meta, packing=self.req["packing"], channels=list(self.names), lat=self.lat.tolist(), lon=self.lon.tolist(),
                        time_step_s=self.step.total_seconds(), start_time=iso(self.start), source=self.source,
                        leads=[k for k, _ in self.leads], valid_times=[iso(t) for _, t in self.leads], files=self.files,
                        n_bad=self.n_bad if self.width == 2 else None)
        tmp = self.dir / (MANIFEST + ".part")
        tmp.write_text(json.dumps(manifest, indent=1))
        tmp.replace(self.dir / MANIFEST)
        ens.archive = MemberArchive(self.dir, manifest)
        ens.paths.extend(ens.archive.paths)

    def close(self) -> None:
        """The save threads ended, also after an error (the files whose copies are queued are still written), and no ``.part`` file left."""
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
            for part in self.dir.glob("*.part") if self.dir is not None else ():
                try:
                    part.unlink()
                except OSError:
                    pass


# ---- reading ------------------------------------------------------------------------------------------------------------------------------ #
def open(directory) -> "MemberArchive":                    # noqa: A001 (``archive.open(dir)``, as ``Climate.open``)
    """The archive ``ensemble_forecast(archive=...)`` wrote under ``directory`` (the one that holds ``manifest.json``)."""
    return MemberArchive(directory)


class MemberArchive:
    """A forecast's members on disk: ``manifest.json`` and one netCDF-3 file per (member, saved lead), packed (``int16``) or plain
    (``float32``).  ``paths``: its files; ``info()``: a summary; ``member(m, k)``: a decoded DataArray; ``states(k, device)``: the M device
    states of entry k; ``replay(**request)``: the products of ``ensemble_forecast`` from the files, without a model."""

    def __init__(self, directory, manifest=None):
        import json
        self.dir = Path(directory)
        if manifest is None:
            f = self.dir / MANIFEST
            if not f.exists():
                raise ValueError(f"archive: no {MANIFEST} under {self.dir}")
            manifest = json.loads(f.read_text())
        need = ("model", "n_members", "packing", "channels", "lat", "lon", "time_step_s", "start_time", "leads", "valid_times", "files")
        missing = [k for k in need if k not in manifest]
        if missing or manifest["packing"] not in PACKINGS:
            raise ValueError(f"archive: {self.dir / MANIFEST} lacks {missing} or names an unknown packing")
        self.manifest = manifest
        self.model_name, self.M, self.packing = manifest["model"], int(manifest["n_members"]), manifest["packing"]
        self.channels, self.leads = list(manifest["channels"]), [int(k) for k in manifest["leads"]]
        self.lat, self.lon = np.asarray(manifest["lat"], np.float64), np.asarray(manifest["lon"], np.float64)
        import datetime
        self.start_time = datetime.datetime.fromisoformat(manifest["start_time"])
        self.valid_times = [datetime.datetime.fromisoformat(t) for t in manifest["valid_times"]]
        self.time_step = datetime.timedelta(seconds=float(manifest["time_step_s"]))
        if len(manifest["files"]) != len(self.leads) or any(len(row) != self.M for row in manifest["files"]):
            raise ValueError(f"archive: {self.dir / MANIFEST} does not list one file per member and lead")

    @property
    def paths(self) -> list:
        return [str(self.dir / f) for row in self.manifest["files"] for f in row]

    @property
    def complete(self) -> bool:
        """Every lead from 0 is held (``save_every=1``): what tracks and time windows need."""
        return self.leads == list(range(len(self.leads)))

    def info(self) -> dict:
        m = self.manifest
        width = 2 if self.packing == "int16" else 4
        bad = m.get("n_bad")
        return dict(model=self.model_name, n_members=self.M, seed=m.get("seed"), perturbation=m.get("perturbation"), packing=self.packing,
                    channels=list(self.channels), grid=(self.lat.size, self.lon.size), time_step_h=self.time_step.total_seconds() / 3600.0,
                    start_time=m["start_time"], leads=list(self.leads), valid_times=list(m["valid_times"]), n_files=len(self.paths),
                    payload_bytes=width * len(self.channels) * self.lat.size * self.lon.size * self.M * len(self.leads),
                    n_bad=None if bad is None else int(sum(v for lead in bad for mem in lead for v in mem)), complete=self.complete)

    def path(self, m: int, k: int):
        if not (0 <= int(m) < self.M and 0 <= int(k) < len(self.leads)):
            raise IndexError(f"archive: member {m}, entry {k} of {self.M} members and {len(self.leads)} saved leads")
        return self.dir / self.manifest["files"][int(k)][int(m)]

    def member(self, m: int, k: int):
        """Member ``m`` at entry ``k`` of the saved leads as a decoded DataArray (time, channel, lat, lon)."""
        from .labeled import open_dataarray
        return open_dataarray(self.path(m, k))

    def states(self, k: int, device="cuda:0") -> tuple:
        """(valid time, the M device states (nc, H, W) of entry ``k``).  The bytes of a file go to pinned memory and to the device as they
        are -- half of a float32 state for ``int16`` -- and are unpacked (``pack_unpack``) or swapped (``skio_bswap32``) there."""
        import torch
        from . import deliver
        from .ncio import PACK_TABLES, read_dataarray_netcdf3, read_payload_netcdf3
        nc, H, W = len(self.channels), self.lat.size, self.lon.size
        dev, out = torch.device(device), []
        for m in range(self.M):
            if self.packing == "int16":
                p = read_dataarray_netcdf3(self.path(m, k), raw=True).packed
                rec = np.zeros(nc, ENTRY)
                rec["scale"], rec["offset"] = p.scale[0], p.offset[0]
                host = torch.from_numpy(p.image.copy()).pin_memory()
                st = torch.empty((nc, H, W), dtype=torch.float32, device=dev)
                run_unpack(host.to(dev, non_blocking=True), table_tensor(rec, dev), st)
            else:
                be = np.ascontiguousarray(read_payload_netcdf3(self.path(m, k))).reshape(-1).view(np.uint8)
                host = torch.from_numpy(be.copy()).pin_memory()
                st = host.to(dev, non_blocking=True).view(torch.int32)
                deliver.bswap32(st, st, torch.cuda.current_stream(dev))
                st = st.view(torch.float32).view(nc, H, W)
            if tuple(st.shape) != (nc, H, W):
                raise ValueError(f"archive: {self.path(m, k)} does not hold ({nc}, {H}, {W})")
            out.append(st)
        return self.valid_times[k], out

    def replay(self, device="cuda:0", **request):
        """``ensemble_forecast`` on the members of the archive: the same plan, the same stage list, no model and no weights
        (``replay`` below has the arguments)."""
        return replay(self, device=device, **request)


class _Stub:
    """What the stages read of a model, from the manifest: grid, channel names, time step, device."""

    def __init__(self, arch, device):
        import torch
        from types import SimpleNamespace
        self.grid = SimpleNamespace(lat=arch.lat, lon=arch.lon)
        self.out_channel_names = self.in_channel_names = list(arch.channels)
        self.time_step, self.device = arch.time_step, torch.device(device)


class ArchiveMembers:
    """The member source of a replay: ``advance(k)`` gives entry k of the archive's saved leads, ``close()`` has nothing to end."""

    def __init__(self, arch, device):
        self.arch, self.device = arch, device

    def advance(self, k: int) -> tuple:
        return self.arch.states(k, self.device)

    def close(self) -> None:
        pass


REPLAY_ARGS = ("products", "exceed", "quantiles", "channels", "keep_members", "derived", "derived_surface", "vertical", "grid", "regrid_method", "scores",
               "truth", "climatology", "events", "neighbourhoods_km", "points", "point_channels", "point_method", "aggregates", "neighbourhood", "extremes",
               "scenarios", "spectra", "objects", "tracks", "track_config", "save", "save_config")


def replay(arch, device="cuda:0", **request):
    """The products of ``ensemble_forecast`` from the members of ``arch`` (a ``MemberArchive`` or its directory): every argument that
    only reads states -- ``REPLAY_ARGS`` -- with the meaning it has there; the saved leads of the archive are the leads of the replay.
    Refused before any file is opened for data: an argument that makes members (perturbation, breeding, stochastic ...), ``scores=True``
    without ``truth=``, ``scenarios`` with ``normalise="std"``, a product that needs a channel the archive does not hold, and ``tracks``
    or ``aggregates`` when the archive does not hold every lead from 0.  Returns an ``ensemble.EnsembleForecast``."""
    from types import SimpleNamespace
    from . import ensemble
    from .leads import require_gpu
    arch = arch if isinstance(arch, MemberArchive) else MemberArchive(arch)
    unknown = [k for k in request if k not in REPLAY_ARGS]
    if unknown:
        raise ValueError(f"replay: {unknown} are not arguments of a replay; it reads states and takes {list(REPLAY_ARGS)}")
    r = dict(products=("mean", "spread"), exceed=None, quantiles=None, channels=None, keep_members=False, scores=False, truth=None,
             climatology=None, tracks=False, track_config=None, save=False, save_config=None)
    r.update(request)
    if r["scores"] and r["truth"] is None:
        raise ValueError("replay: scores=True needs truth=: an archive has no data source to fetch an analysis from")
    if (r.get("scenarios") or {}).get("normalise") == "std":
        raise ValueError('replay: scenarios with normalise="std" needs the model\'s channel_std, which an archive does not hold')
    if not arch.complete:
        for what in ("tracks", "aggregates"):
            if r.get(what):
                raise ValueError(f"replay: {what} needs every lead from 0; the archive holds the leads {arch.leads}")
    gm = SimpleNamespace(model=_Stub(arch, device), model_name=arch.model_name, source_label=arch.manifest.get("source", "file"),
                         data_source=None)
    n_steps = len(arch.leads) - 1
    extra = {k: r[k] for k in ("events", "neighbourhoods_km", "points", "point_channels", "point_method", "scenarios", "spectra", "objects",
                               "extremes", "aggregates", "neighbourhood", "derived_surface", "vertical", "derived", "grid", "regrid_method") if k in r}
    try:
        p = ensemble.plan_request(gm.model, n_steps, arch.M, int(arch.manifest.get("seed") or 0), r["products"], r["exceed"], r["quantiles"],
                                  r["channels"], 1, r["keep_members"], scores=r["scores"], **extra)
    except ValueError as e:
        raise ValueError(f"replay: {e} (the archive holds the channels {arch.channels})") from e
    require_gpu(device, "replay unpacks and reduces the members with HIP kernels: it needs a GPU", present=True)
    todo, families = ensemble.stages(gm, p, arch.start_time, r["truth"], r["climatology"], r["scores"], r["tracks"], r["track_config"])
    return ensemble.drive(gm, p, todo, families, ArchiveMembers(arch, device), n_steps, r["save"], r["save_config"],
                          float(arch.manifest.get("perturb_scale") or 0.0))
