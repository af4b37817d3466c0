"""GPU input pipeline and output post-processing around the denoising path.

f1  ``GpuImageLoader``: the reference feeds training from a single-threaded PIL/torchvision dataset
    (utils/datasets/dataset.py:15-50 with DataLoader(num_workers=0), scripts/train.py:35).  Here the host only
    decodes PNGs into pinned uint8 staging buffers (a prefetch thread), copies them on a side stream, and ONE
    kernel does ToTensor + bilinear Resize(antialias=False) + Normalize for the whole batch.
f2  ``gray_mask_batch`` / ``agent_mask_batch``: get_gray_image's histogram-peak background detection and +-0.1
    mask (vectorization/utils/image_utils.py:13-43, its per-pixel Python loop at :40 is the vectoriser's first
    bottleneck) and extract_agents' threshold (vectorization/direct/extract_vehicles.py:136-148) for a batch of
    generated images that is still on the GPU.
"""
from __future__ import annotations

import glob
import queue
import threading

import numpy as np
import torch

from . import _lib, sharding


def resize_normalize(images: torch.Tensor, size, mean=0.5, std=0.5) -> torch.Tensor:
    """[N, Hs, Ws, C] (GPU) -> fp32 [N, C, H, W] = Normalize(Resize(.)) of
    uint8: a decoded image through ToTensor (/ 255)                         (dataset.py:43-45)
    float32: the .pkl branch's `fig_tensor`, permuted HWC -> CHW and used as is  (dataset.py:37-41)"""
    if not images.is_cuda or images.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("resize_normalize: expects a uint8 or float32 GPU tensor [N, H, W, C] (no CPU fallback)")
    n, hs, ws, c = images.shape
    out = torch.empty((n, c, size[0], size[1]), dtype=torch.float32, device=images.device)
    x = images.contiguous()
    lib = _lib.load()
    fn = lib.dsg_resize_normalize_u8 if x.dtype == torch.uint8 else lib.dsg_resize_normalize_f32
    with torch.cuda.device(x.device):
        _lib.check(fn(x.data_ptr(), n, hs, ws, c, _lib.ptr(out), size[0], size[1], float(mean), float(std),
                      _lib.stream_ptr(x.device)))
    return out


_warned_pickles = set()


def load_sample_pickle(path, trust_pickles=False):
    """A ``.pkl`` sample of the reference's dataset (utils/datasets/dataset.py:31-41): ``{"fig_tensor": tensor}``.  Read with
    ``torch.load(weights_only=True)`` -- such a dict needs nothing more, and a data directory is not a place to run code from.
    ONLY the restricted unpickler's refusal of a global it does not allow (``pickle.UnpicklingError``) makes a file "not a
    usable dict" (returns None, with one warning per file that names it and ``trust_pickles=True``): the reference skips a
    non-dict pickle for the next file (dataset.py:37-39) and so do the callers.  A truncated or corrupt file, an I/O error
    -- anything else -- propagates: the reference's ``torch.load`` would raise there too, and silently training on a
    neighbour instead would duplicate samples.  ``trust_pickles=True`` falls back to full unpickling -- which executes code
    from the file -- for pickles that need it."""
    import pickle
    with open(path, "rb") as fh:
        try:
            return torch.load(fh, weights_only=True)
        except pickle.UnpicklingError as e:
            if not trust_pickles:
                if path not in _warned_pickles:
                    _warned_pickles.add(path)
                    import warnings
                    warnings.warn(f"{path}: skipped -- the restricted unpickler refused it ({str(e).splitlines()[0][:120]}); "
                                  "pass trust_pickles=True to unpickle it fully (that executes code from the file)",
                                  RuntimeWarning, stacklevel=2)
                return None
            fh.seek(0)
            return torch.load(fh, weights_only=False)


class GpuImageLoader:
    """Iterates batches of normalised fp32 [B, C, H, W] GPU tensors from the files ``Image_Dataset`` reads
    (utils/datasets/dataset.py:15-50): PNG / any PIL image, or ``.pkl`` with a ``fig_tensor`` [H, W, C] float entry
    (a pickle that is not a dict falls through to the next file, dataset.py:39-40).

    Host side: a batch's files are decoded in parallel, each image straight into its row of a pinned staging buffer from a
    small ring that is allocated once and reused (a slot is rewritten only after the H2D copy that read it has completed:
    an event per slot); batches come out in the sampler's order whatever order the decodes finish in.  The H2D copy and
    the one resize + normalise kernel of a batch are issued by the producer thread on a side stream as soon as the batch is
    decoded, `prefetch` batches ahead of the consumer.  PNG batches go through the library's own decoder
    (``dsg_png_decode_batch``, csrc/pngdec.hip: `workers` native threads, no GIL); everything else -- other formats, .pkl
    samples, PNG variants the decoder leaves alone -- through a pool of `workers` Python threads over PIL (which scales
    poorly: its chunk loop holds the GIL).  One PIL thread gives 145-326 images/s on 512x512 RGB PNGs -- below what a
    training step consumes (249 images/s fp32, 699 bf16); ``decode_rate()`` measures the pool (5800-6200 images/s with 16
    workers on the GPU box).

    Under data parallelism (`rank`, `world`) it follows accelerate's prepared loader exactly like
    ``training._ShardedLoader`` (sharding.py): ONE shuffled order per epoch on every rank -- rank 0 draws the epoch's
    seed, broadcasts it when a process group exists (`seed=None`), or all ranks derive it from `seed + epoch` -- rank r
    takes batches r, r + W, ..., and a ragged tail is completed from the start of the order so that every rank runs
    ``len(loader)`` full-size steps (a rank short of one batch would never join the last gradient all-reduce)."""

    def __init__(self, pattern_or_files, size, batch_size, shuffle=True, seed=0, device="cuda", prefetch=2,
                 rank=0, world=1, drop_last=False, trust_pickles=False, workers=None, native_png=True):
        self.files = sorted(glob.glob(pattern_or_files)) if isinstance(pattern_or_files, str) else list(
            pattern_or_files)
        self.size, self.bs, self.shuffle, self.seed = tuple(size), batch_size, shuffle, seed
        self.device = torch.device(device)
        self.prefetch, self.rank, self.world, self.drop_last = prefetch, rank, world, drop_last
        # .pkl samples are read with torch.load(weights_only=True) (a {"fig_tensor": tensor} dict needs nothing more);
        # trust_pickles=True falls back to full unpickling -- which runs code from the data directory -- for other pickles
        self.trust_pickles = bool(trust_pickles)
        import os
        self.workers = max(1, int(workers)) if workers is not None else max(1, min(16, (os.cpu_count() or 2) - 1))
        self.native_png = bool(native_png)   # False: every file through PIL (the A/B switch of decode_rate)
        self.epoch = 0
        self.epoch_seed = None
        self._copy_stream = None
        self._pool = None
        self._ring = None        # [{"buf": pinned tensor [B, H, W, C], "event": copy-finished event or None}] * (prefetch + 2)
        self._ring_key = None
        self._slot = 0

    def __len__(self):
        return sharding.steps_per_epoch(len(self.files), self.bs, self.world, self.drop_last)

    def _batches(self):
        idx = np.arange(len(self.files))
        if self.shuffle:
            self.epoch_seed = (sharding.broadcast_epoch_seed(self.rank, self.world, self.device) if self.seed is None
                               else self.seed + self.epoch)
            np.random.default_rng(self.epoch_seed).shuffle(idx)
        return sharding.shard_batches(idx.tolist(), self.bs, self.rank, self.world, self.drop_last)

    def _load_one(self, i):
        """One file as an HWC array: uint8 for images, float32 for the .pkl branch.  A .pkl that does not hold a dict is
        skipped for the next file (the reference's dataset does the same, utils/datasets/dataset.py:31-36); after one full
        round of the file list without a usable file this raises instead of recursing for ever."""
        for k in range(len(self.files)):
            f = self.files[(i + k) % len(self.files)]
            if not f.lower().endswith(".pkl"):
                from PIL import Image
                with Image.open(f) as im:
                    a = np.asarray(im)
                return a[:, :, None] if a.ndim == 2 else a
            dd = load_sample_pickle(f, self.trust_pickles)
            if isinstance(dd, dict):
                return np.ascontiguousarray(dd["fig_tensor"][:, :, :].float().numpy())
        raise IndexError(f"GpuImageLoader: no usable sample among {len(self.files)} files (every .pkl was refused by the "
                         "restricted unpickler or holds a non-dict object; see trust_pickles)")

    # ---- decode pool + pinned staging ring -----------------------------------------------------------------------
    def _executor(self):
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="dsg-decode")
        return self._pool

    def _staging(self, shape, dtype):
        """The next slot of the ring for batches of `shape` / `dtype` (re-made when a batch of another shape arrives);
        waits for the H2D copy that last read the slot."""
        key = (tuple(shape[1:]), dtype)
        if self._ring is None or self._ring_key != key:
            pin = torch.cuda.is_available()
            tdt = torch.uint8 if dtype == np.uint8 else torch.float32
            self._ring = [{"buf": torch.empty((self.bs,) + key[0], dtype=tdt, pin_memory=pin), "event": None}
                          for _ in range(self.prefetch + 2)]
            self._ring_key, self._slot = key, 0
        slot = self._ring[self._slot]
        self._slot = (self._slot + 1) % len(self._ring)
        if slot["event"] is not None:
            slot["event"].synchronize()
            slot["event"] = None
        return slot

    def _decode_native(self, ids):
        """A batch of .png files through the library's native decoder (``dsg_png_decode_batch``: `workers` C++ threads, the
        whole call outside the GIL, rows written straight into the pinned slot).  Files it does not take (16-bit, palette,
        interlaced, damaged: a per-file status) are read with PIL into the same rows.  None: not a pure-PNG batch, or the
        first file is not one the decoder handles -- the generic pool path decodes the batch."""
        import ctypes as C
        files = [self.files[i] for i in ids]
        if not self.native_png or not all(f.lower().endswith(".png") for f in files):
            return None
        lib = _lib.load()
        h, w, c = C.c_int32(), C.c_int32(), C.c_int32()
        if lib.dsg_png_probe(files[0].encode(), C.byref(h), C.byref(w), C.byref(c)) != 0:
            return None
        n = len(files)
        slot = self._staging((n, h.value, w.value, c.value), np.uint8)
        paths = (C.c_char_p * n)(*[f.encode() for f in files])
        status = (C.c_int32 * n)()
        _lib.check(lib.dsg_png_decode_batch(paths, n, slot["buf"].data_ptr(), h.value, w.value, c.value, self.workers, status))
        view = None
        for j, st in enumerate(status):
            if st != 0:     # this file goes through PIL (which also raises the proper error for a damaged file)
                a = self._load_one(ids[j])
                view = slot["buf"].numpy() if view is None else view
                if a.shape != view.shape[1:] or a.dtype != np.uint8:
                    raise ValueError("GpuImageLoader: images of one batch must share a shape")
                np.copyto(view[j], a)
        return slot, n

    def _decode(self, ids):
        """Decode one batch on the pool: returns (slot, rows) -- the pinned [rows, H, W, C] staging view is slot["buf"][:rows]."""
        ids = list(ids)
        native = self._decode_native(ids)
        if native is not None:
            return native
        first = self._load_one(ids[0])    # (names the batch's shape / dtype; the other members are decoded by the pool)
        mixed = {}

        def work(j, i, slot_np):
            a = first if j == 0 else self._load_one(i)
            if a.shape != slot_np.shape[1:]:
                raise ValueError("GpuImageLoader: images of one batch must share a shape")
            if a.dtype != slot_np.dtype:
                if slot_np.dtype == np.uint8:     # a .pkl member in a PNG batch: the whole batch must travel as float32
                    mixed[j] = a
                    return
                a = a.astype(np.float32) / np.float32(255) if a.dtype == np.uint8 else a.astype(np.float32, copy=False)
            np.copyto(slot_np[j], a)

        dtype = np.uint8 if first.dtype == np.uint8 else np.float32
        slot = self._staging((len(ids),) + first.shape, dtype)
        view = slot["buf"].numpy()
        list(self._executor().map(lambda ji: work(ji[0], ji[1], view), enumerate(ids)))
        if mixed:   # (rare: ToTensor's / 255 on the host for the uint8 members, as a batch of float32)
            slot = self._staging((len(ids),) + first.shape, np.float32)
            fview = slot["buf"].numpy()
            for j in range(len(ids)):
                fview[j] = mixed[j].astype(np.float32, copy=False) if j in mixed else view[j].astype(np.float32) / np.float32(255)
        return slot, len(ids)

    def decode_rate(self, batches: int = 4):
        """Images / s of the host side alone (decode pool into pinned staging, no GPU work): what the loader can feed."""
        import time
        todo = self._batches()[:batches]
        self._decode(todo[0])          # (pool start-up, ring allocation)
        t0 = time.perf_counter()
        n = sum(self._decode(ids)[1] for ids in todo)
        return n / (time.perf_counter() - t0)

    def __iter__(self):
        """The producer thread does everything that can run ahead of the consumer: decode into a pinned slot, H2D copy and
        the resize + normalise kernel on the loader's side stream, an event behind them -- `prefetch` finished batches wait
        in the queue.  The consumer only makes its stream wait for the batch's event (no copy is ever issued from the
        training thread, none waits for the training stream)."""
        q: "queue.Queue" = queue.Queue(maxsize=self.prefetch)
        batches = self._batches()
        self.epoch += 1
        stop = threading.Event()
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        side = self._copy_stream

        def producer():
            try:
                for ids in batches:
                    if stop.is_set():
                        return
                    slot, rows = self._decode(ids)
                    with torch.cuda.stream(side):
                        dev = slot["buf"][:rows].to(self.device, non_blocking=True)
                        copied = torch.cuda.Event()
                        copied.record(side)
                        slot["event"] = copied   # the slot is rewritten only after this copy has read it (ring of prefetch + 2)
                        out = resize_normalize(dev, self.size)
                        ready = torch.cuda.Event()
                        ready.record(side)
                    q.put((out, ready))
            except Exception as e:  # surfaced in the consumer
                q.put(e)
            q.put(None)

        worker = threading.Thread(target=producer, daemon=True)
        worker.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, Exception):
                    raise item
                out, ready = item
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ready)
                out.record_stream(cur)      # (allocated on the side stream, used on the consumer's)
                yield out
        finally:
            # a consumer that stops early: tell the producer, keep the queue drained so that it cannot block on a full queue, and
            # JOIN it -- when the iterator is gone no thread of this loader is still decoding, copying or launching kernels
            stop.set()
            while worker.is_alive():
                try:
                    q.get(timeout=0.05)
                except queue.Empty:
                    pass
            worker.join()


# --------------------------------------------------------------------------------------------------
# f2: output post-processing
# --------------------------------------------------------------------------------------------------
_U = np.arange(256)
# np.histogram(bins=256, range=(0,1)) bin of the value u/255 (float64), for every byte value u
_BIN_OF_U = np.array([int(np.argmax(np.histogram(np.array([u / 255.0]), bins=256, range=(0, 1))[0])) for u in _U])
_EDGES = np.histogram(np.array([0.0]), bins=256, range=(0, 1))[1]


def histograms_u8(images_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [N, H, W, C] (GPU) -> int64 [N, C, 256] byte histograms."""
    n, h, w, c = images_u8.shape
    hist = torch.empty((n, c, 256), dtype=torch.int32, device=images_u8.device)
    x = images_u8.contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dsg_hist_u8(x.data_ptr(), n, h * w, c, hist.data_ptr(), _lib.stream_ptr(x.device)))
    return hist


def _mask_lut(images_u8, luts, ch0, ch1, on, off):
    n, h, w, c = images_u8.shape
    lut = torch.from_numpy(np.ascontiguousarray(luts, dtype=np.uint8)).to(images_u8.device)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=images_u8.device)
    x = images_u8.contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dsg_mask_lut_u8(x.data_ptr(), n, h * w, c, ch0, ch1, lut.data_ptr(), on, off,
                                              out.data_ptr(), _lib.stream_ptr(x.device)))
    return out


def gray_mask_batch(images_u8: torch.Tensor) -> torch.Tensor:
    """get_gray_image for a batch: uint8 [N, H, W, >=2] (GPU) -> uint8 [N, H, W] mask (0 = background, 255 = lane).
    The histogram runs on the GPU; the 256-entry decision tables are built on the host with the reference's float64
    arithmetic (peak bin edge mx, |u/255 - mx| <= 0.1), so the mask is bit-identical to the reference loop."""
    if not images_u8.is_cuda or images_u8.dtype != torch.uint8:
        raise RuntimeError("gray_mask_batch: expects a uint8 GPU tensor [N, H, W, C] (no CPU fallback)")
    hist_u = histograms_u8(images_u8)[:, :2].cpu().numpy().astype(np.int64)  # [N, 2, 256]
    n = hist_u.shape[0]
    luts = np.zeros((n, 2, 256), np.uint8)
    vals = _U / 255.0
    for i in range(n):
        for ch in range(2):
            hb = np.bincount(_BIN_OF_U, weights=hist_u[i, ch], minlength=256)
            m = _EDGES[int(np.argmax(hb))]
            luts[i, ch] = np.fabs(vals - m) <= 0.1
    return _mask_lut(images_u8, luts, 0, 1, 0, 255)  # both channels near the peak -> background (0)


def agent_mask_batch(images_u8: torch.Tensor, channel: int = 2, thresh: int = 100) -> torch.Tensor:
    """extract_agents' binarisation for a batch of generated uint8 images [N, H, W, C] (GPU): the reference
    re-reads the PNG as float32 /255, multiplies by 255, truncates to uint8 and thresholds at 100."""
    if not images_u8.is_cuda or images_u8.dtype != torch.uint8:
        raise RuntimeError("agent_mask_batch: expects a uint8 GPU tensor [N, H, W, C] (no CPU fallback)")
    f = (_U.astype(np.float32) / np.float32(255)).astype(np.float32)
    lut1 = ((f * 255).astype(np.uint8) > thresh).astype(np.uint8)
    luts = np.broadcast_to(np.stack([lut1, lut1])[None], (images_u8.shape[0], 2, 256))
    return _mask_lut(images_u8, luts, channel, -1, 255, 0)


# --------------------------------------------------------------------------------------------------
# f2, continued: the skeleton stage (extract_network.py:270-277) -- csrc/skeleton.hip
# --------------------------------------------------------------------------------------------------
DEFAULT_NODE_CAP = 4096    # rows of skeleton_nodes_batch's coordinate list per image (a 512 x 512 lane skeleton has a few dozen nodes)


def zhang_suen_lut() -> np.ndarray:
    """uint8 [256], the default thinning table (Zhang & Suen, CACM 27(3), 1984), indexed by an on pixel's neighbour code
    NW 1 + N 2 + NE 4 + E 8 + SE 16 + S 32 + SW 64 + W 128 (N = smaller index on axis 0, W = smaller index on axis 1).
    Bit 0 = delete in the first sub-iteration, bit 1 = delete in the second.  A code is marked when 2 <= B <= 6 (B on
    neighbours) and A = 1 (A off -> on steps walking N, NE, E, SE, S, SW, W, NW, N); bit 0 also needs N.E.S = 0 and E.S.W = 0,
    bit 1 needs N.E.W = 0 and N.S.W = 0.  Parity with scikit-image's own table is unpinned (scikit-image is not a dependency):
    ``skeletonize_batch(lut=...)`` takes any table of this layout."""
    code = np.arange(256)
    nw, n, ne, e, se, s, sw, w = [(code >> k) & 1 for k in range(8)]
    walk = np.stack([n, ne, e, se, s, sw, w, nw])
    b = walk.sum(0)
    a = ((walk == 0) & (np.roll(walk, -1, axis=0) == 1)).sum(0)
    marked = (b >= 2) & (b <= 6) & (a == 1)
    first = marked & (n * e * s == 0) & (e * s * w == 0)
    second = marked & (n * e * w == 0) & (n * s * w == 0)
    return (first * 1 + second * 2).astype(np.uint8)


_default_thin_lut = {}   # device -> the default table on it (uploaded once: a later call copies nothing and can be captured)


def _thin_lut_on(device, lut):
    if lut is None:
        t = _default_thin_lut.get(device)
        if t is None:
            t = _default_thin_lut[device] = torch.from_numpy(zhang_suen_lut()).to(device)
        return t
    a = np.asarray(lut)
    if a.shape != (256,) or not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 3:
        raise ValueError("skeletonize_batch: lut must hold 256 integers in 0..3 (bit 0: first sub-iteration, bit 1: second)")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(device)


def skeletonize_batch(mask_u8: torch.Tensor, lut=None, max_iters=None, return_iters=False):
    """``morphology.skeletonize`` of extract_network (vectorization/graph/extract_network.py:272) for a batch that is still on
    the GPU: uint8 [N, H, W] (non-zero = on) -> uint8 [N, H, W] skeleton of 0 / 1, in ONE launch (one workgroup per image, the
    image bit-packed in LDS, iterated to convergence there).  With ``return_iters`` also int32 [N], the iterations each image
    took, the last idle one included.

    The algorithm is the two-sub-iteration parallel thinning of Zhang & Suen (1984), driven by ``lut`` (default
    ``zhang_suen_lut()``; any 256 values in 0..3 of that layout, checked on the host).  Parity with scikit-image's table is
    unpinned; a user who has scikit-image can pass its table.  The reference thins ``mask.T``: with the default table the
    result is the same (transposed) either way; with a custom table it may not be -- transpose the input to follow it.

    ``max_iters`` (default H + W) bounds the loop.  An image that has not converged by then is returned as far as it got
    and its iteration count is -1: with ``return_iters`` that raises, without it nothing is read back (the default path makes
    no device-to-host copy).  Under stream capture (``torch.cuda.graph``): the default table is uploaded to a device on the
    first call that uses it there, so make one call outside the capture first; a custom ``lut`` is uploaded on every call and
    cannot be captured.  Images whose packed form exceeds one workgroup's LDS (beyond about 600 x 600: 608 x 608 fits, 640 x 640 does not) are refused."""
    if not isinstance(mask_u8, torch.Tensor) or not mask_u8.is_cuda or mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3:
        raise RuntimeError("skeletonize_batch: expects a uint8 GPU tensor [N, H, W] (no CPU fallback)")
    n, h, w = mask_u8.shape
    table = _thin_lut_on(mask_u8.device, lut)
    x = mask_u8.contiguous()
    skel = torch.empty((n, h, w), dtype=torch.uint8, device=x.device)
    iters = torch.empty((n,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dsg_thin_lut_u8(x.data_ptr(), n, h, w, table.data_ptr(), int(h + w if max_iters is None else max_iters),
                                              skel.data_ptr(), iters.data_ptr(), _lib.stream_ptr(x.device)))
    if not return_iters:
        return skel
    if bool((iters < 0).any().item()):
        raise RuntimeError(f"skeletonize_batch: images {torch.nonzero(iters < 0).flatten().tolist()} had not converged after "
                           f"{int(h + w if max_iters is None else max_iters)} iterations")
    return skel, iters


def skeleton_nodes_batch(skel_u8: torch.Tensor, cap=None, return_class=False):
    """``zhang_suen_node_detection`` (vectorization/graph/extract_network.py:34-93, called at :240) for a batch on the GPU:
    uint8 [N, H, W] (non-zero = on; any image is legal, not only a skeleton) -> (coords int32 [N, cap, 2], counts int32 [N]).
    A node is an on pixel whose A (off -> on steps walking N, NE, E, SE, S, SW, W, NW, N, outside = off) is 1 (end point) or
    >= 3 (branching point).  ``coords[i, :k]`` are the (axis-0 index, axis-1 index) pairs of image i in row-major order of the
    array as given -- the reference's list order -- with k = min(counts[i], cap); the rows behind them are -1.
    ``counts[i]`` is always the TRUE number of nodes: nothing is read back here, so the caller compares ``counts`` with
    ``cap`` (default ``DEFAULT_NODE_CAP`` = 4096) and calls again with a larger one if a list was cut.
    With ``return_class`` also uint8 [N, H, W]: 0 = not a node, else A."""
    if not isinstance(skel_u8, torch.Tensor) or not skel_u8.is_cuda or skel_u8.dtype != torch.uint8 or skel_u8.dim() != 3:
        raise RuntimeError("skeleton_nodes_batch: expects a uint8 GPU tensor [N, H, W] (no CPU fallback)")
    n, h, w = skel_u8.shape
    cap = DEFAULT_NODE_CAP if cap is None else int(cap)
    if cap < 0:
        raise ValueError("skeleton_nodes_batch: cap must not be negative")
    x = skel_u8.contiguous()
    coords = torch.full((n, cap, 2), -1, dtype=torch.int32, device=x.device)
    counts = torch.empty((n,), dtype=torch.int32, device=x.device)
    cls = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_class else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dsg_skel_nodes_u8(x.data_ptr(), n, h, w, None if cls is None else cls.data_ptr(),
                                                coords.data_ptr() if cap else None, cap, counts.data_ptr(),
                                                _lib.stream_ptr(x.device)))
    return (coords, counts, cls) if return_class else (coords, counts)


def lane_skeleton_batch(images_u8: torch.Tensor):
    """A batch of generated uint8 images [N, H, W, >=2] (GPU) -> (mask, skeleton, coords, counts): ``gray_mask_batch``, then
    ``skeletonize_batch``, then ``skeleton_nodes_batch`` with their defaults.  Stands in for the head of the reference's lane
    extraction: get_gray_image (vectorization/utils/image_utils.py:13-43), ``morphology.skeletonize`` and
    ``zhang_suen_node_detection`` (vectorization/graph/extract_network.py:270-277, :272 and :240).  The reference thins and
    scans ``mask.T``; here the arrays keep the image's own orientation (the default table gives the same skeleton either way),
    so swap the two coordinates -- and re-sort -- to get the reference's (x, y) list.  This is the list after extract_network.py:240;
    ``lane_nodes_batch`` goes on to the one ``connect_graph`` works with (dense nodes merged in, :241-242).  find_paths and what
    follows is host graph code and not part of this engine."""
    mask = gray_mask_batch(images_u8)
    skel = skeletonize_batch(mask)
    coords, counts = skeleton_nodes_batch(skel)
    return mask, skel, coords, counts


# --------------------------------------------------------------------------------------------------
# f2, continued: connected components (extract_network.py:96-122, :241-242; extract_vehicles.py:147-148) -- csrc/ccl.hip
# --------------------------------------------------------------------------------------------------
def ccl_tile_shape():
    """(rows, columns) of the tile one workgroup of the labelling kernel holds in LDS; images larger than that are merged
    across tile borders by a second launch."""
    import ctypes as C
    th, tw = C.c_int32(), C.c_int32()
    _lib.check(_lib.load().dsg_ccl_tile_shape(C.byref(th), C.byref(tw)))
    return th.value, tw.value


def _need(fn, t, dtype, dim):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != dim:
        raise RuntimeError(f"{fn}: expects a {str(dtype).replace('torch.', '')} GPU tensor of {dim} dimensions (no CPU fallback)")
    return t.contiguous()


def label_batch(mask_u8: torch.Tensor, connectivity: int = 1, erode2x2: bool = False):
    """``scipy.ndimage.label`` for a batch on the GPU: uint8 [N, H, W] (non-zero = on) -> (labels int32 [N, H, W], counts
    int32 [N]).  ``connectivity`` 1 = 4 neighbours (scipy's default structure), 2 = 8 (``np.ones((3, 3))``).  Labels are 0 for
    off pixels and 1..counts[i] in scipy's numbering: components in row-major order of their first pixel.  ``erode2x2`` first
    erodes with a 2 x 2 block anchored at the larger indices, ``binary_erosion(np.pad(a, 1), np.ones((2, 2)))[1:-1, 1:-1]``
    (extract_network.py:98), inside the kernel's read of the mask.  H * W <= 2^30; the result is bitwise reproducible.
    Nothing is read back."""
    x = _need("label_batch", mask_u8, torch.uint8, 3)
    n, h, w = x.shape
    import ctypes as C
    lib, need = _lib.load(), C.c_size_t()
    _lib.check(lib.dsg_ccl_workspace_bytes(n, h, w, C.byref(need)))
    labels = torch.empty((n, h, w), dtype=torch.int32, device=x.device)
    counts = torch.empty((n,), dtype=torch.int32, device=x.device)
    ws = torch.empty((need.value // 4,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.dsg_ccl_u8(x.data_ptr(), n, h, w, int(connectivity), int(bool(erode2x2)), labels.data_ptr(),
                                  counts.data_ptr(), ws.data_ptr(), need.value, _lib.stream_ptr(x.device)))
    return labels, counts


def _cap_of(fn, cap):
    cap = DEFAULT_NODE_CAP if cap is None else int(cap)
    if cap < 0:
        raise ValueError(f"{fn}: cap must not be negative")
    return cap


def _stats_raw(fn, labels, counts, cap):
    x, c = _need(fn, labels, torch.int32, 3), _need(fn, counts, torch.int32, 1)
    n, h, w = x.shape
    if c.shape[0] != n:
        raise ValueError(f"{fn}: counts must have one entry per image")
    raw = torch.full((n, cap, 8), 0, dtype=torch.int64, device=x.device)   # one 64-byte dsg_cc_stat per row
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dsg_cc_stats_i32(x.data_ptr(), n, h, w, c.data_ptr(), raw.data_ptr() if cap else None, cap,
                                               _lib.stream_ptr(x.device)))
    return raw, c


def component_stats_batch(labels: torch.Tensor, counts: torch.Tensor, cap=None) -> dict:
    """Per-component statistics of ``label_batch``'s output, rows in label order (label k in row k - 1), ``cap`` rows per image
    (default ``DEFAULT_NODE_CAP``); rows at ``min(counts[i], cap)`` and beyond are zero (area 0).  A dict of views of ONE
    tensor ``raw`` int64 [N, cap, 8], the C struct ``dsg_cc_stat`` (include/dsg.h):
      ``area``    int32 [N, cap]       pixels
      ``bbox``    int32 [N, cap, 4]    r0, c0, r1, c1, half-open like ``scipy.ndimage.find_objects``
      ``sums``    int64 [N, cap, 5]    sum of r, c, r*r, c*c, r*c over the component's pixels (r = axis-0 index)
      ``centers`` int32 [N, cap, 2]    (sum_r // area, sum_c // area) = ``int()`` of ``center_of_mass``; -1 behind the list
    Integer sums: exact and run-to-run identical.  Centroid and second moments follow as sums / area on the caller's side.
    H and W <= 32768."""
    cap = _cap_of("component_stats_batch", cap)
    raw, c = _stats_raw("component_stats_batch", labels, counts, cap)
    n = raw.shape[0]
    words = raw.view(torch.int32).view(n, cap, 16)
    centers = torch.full((n, cap, 2), -1, dtype=torch.int32, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(_lib.load().dsg_cc_centers_i32(raw.data_ptr() if cap else None, c.data_ptr(), n, cap,
                                                 centers.data_ptr() if cap else None, _lib.stream_ptr(raw.device)))
    return {"raw": raw, "area": words[:, :, 0], "bbox": words[:, :, 1:5], "sums": raw[:, :, 3:8], "centers": centers}


def dense_skeleton_nodes_batch(skel_u8: torch.Tensor, cap=None):
    """``find_dense_skeleton_nodes`` (vectorization/graph/extract_network.py:96-103) for a batch on the GPU: uint8 [N, H, W]
    -> (coords int32 [N, cap, 2], counts int32 [N]).  The image is eroded with a 2 x 2 block, labelled with 4-connectivity and
    each component gives the floor of its centre of mass, in label order; rows behind the list are -1, ``counts`` is the true
    number of components (compare it with ``cap``, default ``DEFAULT_NODE_CAP``, as for ``skeleton_nodes_batch``)."""
    x = _need("dense_skeleton_nodes_batch", skel_u8, torch.uint8, 3)
    cap = _cap_of("dense_skeleton_nodes_batch", cap)
    labels, counts = label_batch(x, connectivity=1, erode2x2=True)
    return component_stats_batch(labels, counts, cap)["centers"], counts


def merge_dense_nodes_batch(coords: torch.Tensor, counts: torch.Tensor, dense_coords: torch.Tensor, dense_counts: torch.Tensor,
                            min_distance=5):
    """``add_dense_nodes`` (vectorization/graph/extract_network.py:106-122) for a batch on the GPU: a dense node is kept iff no
    node of ``coords[i, :counts[i]]`` is closer than ``min_distance`` (squared distance < min_distance ** 2, strict), whatever
    dense nodes were kept before it.  Returns (a copy of ``coords`` with the kept nodes appended behind the originals in the
    dense list's order, as far as its rows go; counts + kept).  If ``counts[i]`` exceeds the rows of ``coords`` that list was
    cut already: only the listed nodes are compared and nothing is appended -- compare the returned counts with the cap."""
    fn = "merge_dense_nodes_batch"
    a, ca = _need(fn, coords, torch.int32, 3), _need(fn, counts, torch.int32, 1)
    d, cd = _need(fn, dense_coords, torch.int32, 3), _need(fn, dense_counts, torch.int32, 1)
    n = a.shape[0]
    if a.shape[2] != 2 or d.shape[2] != 2 or d.shape[0] != n or ca.shape[0] != n or cd.shape[0] != n:
        raise ValueError(f"{fn}: expects coords [N, cap, 2], counts [N], dense_coords [N, dense_cap, 2], dense_counts [N]")
    min_d2 = min_distance ** 2
    if min_d2 != int(min_d2) or min_d2 < 0:
        raise ValueError(f"{fn}: min_distance ** 2 must be a non-negative integer (coordinates are integers)")
    out = a.clone()
    out_counts = torch.empty_like(ca)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().dsg_merge_nodes_i32(out.data_ptr() if a.shape[1] else None, ca.data_ptr(), n, a.shape[1],
                                                  d.data_ptr() if d.shape[1] else None, cd.data_ptr(), d.shape[1], int(min_d2),
                                                  out_counts.data_ptr(), _lib.stream_ptr(a.device)))
    return out, out_counts


def lane_nodes_batch(images_u8: torch.Tensor):
    """A batch of generated uint8 images [N, H, W, >=2] (GPU) -> (mask, skeleton, coords, counts): ``lane_skeleton_batch``, then
    ``dense_skeleton_nodes_batch`` on the skeleton and ``merge_dense_nodes_batch`` with their defaults -- the node list
    ``connect_graph`` holds after vectorization/graph/extract_network.py:240-242.  As in ``lane_skeleton_batch`` the arrays keep
    the image's own orientation while the reference works on ``mask.T``: the 2 x 2 block is symmetric under transposition, so
    the SET of dense nodes is the reference's with the two coordinates swapped; only the order of the list differs (components
    are numbered in row-major order of the array as given).  What follows (find_paths, the merge loop) is host graph code."""
    mask, skel, coords, counts = lane_skeleton_batch(images_u8)
    dense, dense_counts = dense_skeleton_nodes_batch(skel)
    coords, counts = merge_dense_nodes_batch(coords, counts, dense, dense_counts)
    return mask, skel, coords, counts


def agent_blobs_batch(images_u8: torch.Tensor, channel: int = 2, thresh: int = 100, cap=None):
    """The blobs of extract_agents' thresholded channel (vectorization/direct/extract_vehicles.py:136-148) for a batch of
    generated uint8 images [N, H, W, C] (GPU): ``agent_mask_batch``, ``label_batch`` with 8-connectivity and
    ``component_stats_batch`` -> (labels int32 [N, H, W], counts int32 [N], stats dict): area, bounding box, centre and the
    sums behind the second moments of every blob.  What this is NOT: the reference goes on with
    ``cv2.findContours(thresh, 1, 2)``, which also returns the contours of holes, and fits ``cv2.minAreaRect`` to each; neither
    is computed here, and parity with OpenCV is unpinned (it is not a dependency).  The table is what a host-side rectangle
    fit starts from; everything from ``minAreaRect`` on stays host code."""
    mask = agent_mask_batch(images_u8, channel, thresh)
    labels, counts = label_batch(mask, connectivity=2)
    return labels, counts, component_stats_batch(labels, counts, cap)
