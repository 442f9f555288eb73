"""Device engines: thin owners of the native handles (include/vtd.h) plus the torch tensors that
serve as their caller-owned device buffers.  torch is plumbing here (allocation, streams); every
FLOP is issued by libvtd_hip.so.
"""
import ctypes as C
import logging
import os
import queue
import sys
import threading

import numpy as np
import torch

from . import _native

logger = logging.getLogger(__name__)

DEFAULT_MAX_BATCH = int(os.environ.get("VTD_MAX_BATCH", "32"))

# Kernel-selection table shipped with the package (include/vtd.h: vtd_*_set_tuning): chosen on an MI355X by tools/tune_table.py,
# loaded into every engine so that all processes / ranks run the same kernels.  VTD_TUNING_FILE points at another table,
# VTD_TUNING=0 ignores tables (every shape is then decided by the in-process timing contest).
TUNING_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning", "gfx950.txt")


def shipped_tuning_text():
    if os.environ.get("VTD_TUNING", "1") == "0":
        return ""
    path = os.environ.get("VTD_TUNING_FILE", TUNING_FILE)
    try:
        with open(path) as f:
            return f.read()
    except OSError:
        return ""


class _Tunable:
    """get / set of a handle's kernel-selection table (kind = 'detector' | 'recognizer')."""

    _kind = None

    def set_tuning(self, text):
        """Replaces table entries; under the engine lock, so a forward / generate in another thread never sees its resolved launch
        slots cleared half way."""
        if text:
            fn = getattr(self.lib, f"vtd_{self._kind}_set_tuning")
            with self.lock:
                _native.check(fn(self.handle, text.encode()), f"vtd_{self._kind}_set_tuning")

    def tuning_text(self):
        fn = getattr(self.lib, f"vtd_{self._kind}_get_tuning")
        need = fn(self.handle, None, 0)
        buf = C.create_string_buffer(int(need))
        fn(self.handle, buf, need)
        return buf.value.decode()

    def tuning(self):
        return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in self.tuning_text().splitlines() if line)}

    @property
    def tuning_measured(self):
        """True when some kernel choice of this engine came from its own timing contest (not from a table)."""
        return bool(getattr(self.lib, f"vtd_{self._kind}_tuning_measured")(self.handle))


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class PinnedPool:
    """Recycles pinned host staging buffers (hipHostMalloc costs far more than the copies they serve).  A buffer is
    handed out again only after `release(buf, event)`, which waits for `event` first: the event recorded after the buffer's
    last GPU use (copy_to_pinned writes through a mapped pointer, so torch cannot know the buffer is busy)."""

    def __init__(self):
        self._free = {}
        self._lock = threading.Lock()

    def take(self, shape, dtype=torch.int32):
        key = (tuple(shape), dtype)
        with self._lock:
            lst = self._free.get(key)
            if lst:
                return lst.pop()
        return torch.empty(shape, dtype=dtype).pin_memory()

    def release(self, t, event):
        """`event`: None only for a buffer no GPU work ever touched."""
        if event is not None:
            event.synchronize()
        with self._lock:
            self._free.setdefault((tuple(t.shape), t.dtype), []).append(t)


PINNED = PinnedPool()


def copy_to_pinned(dst, src):
    """Device tensor -> pinned host tensor on the current stream, by a copy kernel (include/vtd.h vtd_copy_to_pinned_host).  The
    asynchronous memcpy of the detection records -- a few KB on the post-process side stream -- was seen to block the host for a whole
    detector pass, once per drained pipeline; a launch never waits for the GPU.  Falls back to the plain
    asynchronous copy if the buffer is not mapped."""
    nbytes = src.numel() * src.element_size()
    if nbytes >= 16 and dst.is_pinned() and src.is_contiguous() and dst.is_contiguous() and dst.numel() * dst.element_size() == nbytes and \
            _native.require().vtd_copy_to_pinned_host(src.data_ptr(), dst.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream) == 0:
        return
    dst.copy_(src, non_blocking=True)


class DeviceFrames:
    """A batch of equally sized uint8 BGR HWC frames resident in HBM ([n,H,W,3] cuda tensor)."""

    def __init__(self, frames, stream=None):
        """`stream`: upload on that HIP stream (give it pinned host memory and the copy overlaps the previous batch's
        compute); consumers order themselves behind `self.ready`.  Default: the caller's current stream."""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        elif isinstance(frames, (list, tuple)):
            frames = torch.from_numpy(np.ascontiguousarray(np.stack(frames)))
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 [n,H,W,3] (BGR)")
        self.ready = None
        if stream is None or frames.is_cuda:
            self.tensor = frames.to("cuda", non_blocking=True).contiguous()
        else:
            with torch.cuda.stream(stream):
                self.tensor = frames.contiguous().to("cuda", non_blocking=True)
                self.ready = torch.cuda.Event()
                self.ready.record()

    def wait_ready(self):
        """Make the current stream wait for an upload that was issued on another stream (no-op otherwise)."""
        if self.ready is not None:
            torch.cuda.current_stream().wait_event(self.ready)

    @property
    def n(self):
        return self.tensor.shape[0]

    @property
    def height(self):
        return self.tensor.shape[1]

    @property
    def width(self):
        return self.tensor.shape[2]


class DetectorEngine(_Tunable):
    """DBNet on the GPU: reference checkpoint tensors in, [n,1,640,640] probability maps out."""

    _kind = "detector"

    def __init__(self, backbone, state_dict, max_batch=None, options=None):
        self.lib = _native.require()
        self.max_batch = max_batch or DEFAULT_MAX_BATCH
        self.backbone = backbone
        self.lock = threading.Lock()  # a handle is single-stream; detect() may be entered from 4 threads
        h = C.c_void_p()
        _native.check(self.lib.vtd_detector_create(backbone.encode(), self.max_batch, C.byref(h)), "vtd_detector_create")
        self.handle = h
        try:
            for name, value in (options or {}).items():
                _native.check(self.lib.vtd_detector_set_option(h, name.encode(), int(value)), f"vtd_detector_set_option({name})")
            for key, value in state_dict.items():
                if key.endswith("num_batches_tracked"):
                    continue
                arr = np.ascontiguousarray(value.detach().cpu().float().numpy())
                _native.check(self.lib.vtd_detector_set_tensor(h, key.encode(), arr.ctypes.data, arr.size),
                              f"vtd_detector_set_tensor({key})")
            _native.check(self.lib.vtd_detector_finalize(h, _stream_ptr()), "vtd_detector_finalize")
            self.set_tuning(shipped_tuning_text())
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vtd_detector_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def macs_per_frame(self):
        return int(self.lib.vtd_detector_macs_per_frame(self.handle))

    def _set_input(self, x):
        if isinstance(x, DeviceFrames):
            n = x.n
            x.wait_ready()
            _native.check(self.lib.vtd_detector_preprocess(self.handle, C.c_void_p(x.tensor.data_ptr()), n, x.height, x.width,
                                                           _stream_ptr()), "vtd_detector_preprocess")
            return n, x
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (3, 640, 640):
            raise ValueError("DBNet input must be [n,3,640,640] float or a DeviceFrames batch")
        xd = x.to("cuda", torch.float32).contiguous()
        _native.check(self.lib.vtd_detector_set_input_nchw(self.handle, C.c_void_p(xd.data_ptr()), xd.shape[0], _stream_ptr()),
                      "vtd_detector_set_input_nchw")
        return xd.shape[0], xd

    def forward(self, x, want_threshold=False):
        with self.lock:
            n, keep = self._set_input(x)
            prob = torch.empty((n, 1, 640, 640), dtype=torch.float32, device="cuda")
            thr = torch.empty_like(prob) if want_threshold else None
            _native.check(self.lib.vtd_detector_forward(self.handle, n, C.c_void_p(prob.data_ptr()),
                                                        C.c_void_p(thr.data_ptr()) if thr is not None else None, _stream_ptr()),
                          "vtd_detector_forward")
            del keep
            return {"probability": prob, "threshold": thr}

    def forward_features(self, x):
        """P2 (fpn.layer_blocks.3's output) of the input as a new padded-features tensor, ring-padded NHWC fp16 [n,162,162,256] (the
        layout the DB-head training kernels read; include/vtd.h vtd_detector_forward_features).  Needs options fuse_fpn_head=0."""
        with self.lock:
            n, keep = self._set_input(x)
            feats = torch.empty((n, 162, 162, 256), dtype=torch.float16, device="cuda")
            _native.check(self.lib.vtd_detector_forward_features(self.handle, n, C.c_void_p(feats.data_ptr()), _stream_ptr()),
                          "vtd_detector_forward_features")
            del keep
            return feats

    def forward_trunk(self, x):
        """The four trunk taps C2..C5 of the input as new padded-tap tensors, ring-padded NHWC fp16 [n,h+2,w+2,c] with h = w = 160, 80,
        40, 20 (the layout the FPN training kernels read; include/vtd.h vtd_detector_forward_trunk).  Needs options fuse_fpn_head=0."""
        wide = 4 if self.backbone == "resnet50" else 1
        with self.lock:
            n, keep = self._set_input(x)
            taps = [torch.empty((n, (160 >> i) + 2, (160 >> i) + 2, (64 << i) * wide), dtype=torch.float16, device="cuda") for i in range(4)]
            _native.check(self.lib.vtd_detector_forward_trunk(self.handle, n, *(C.c_void_p(t.data_ptr()) for t in taps), _stream_ptr()),
                          "vtd_detector_forward_trunk")
            del keep
            return taps

    def forward_pool(self, x):
        """The pooled stem output of the input (what ResNet's layer1 reads) as a new padded-tap tensor, ring-padded NHWC fp16
        [n,162,162,64] with a zero ring (include/vtd.h vtd_detector_forward_pool).  Only the stem runs."""
        with self.lock:
            n, keep = self._set_input(x)
            tap = torch.empty((n, 162, 162, 64), dtype=torch.float16, device="cuda")
            _native.check(self.lib.vtd_detector_forward_pool(self.handle, n, C.c_void_p(tap.data_ptr()), _stream_ptr()),
                          "vtd_detector_forward_pool")
            del keep
            return tap

    def forward_c2(self, x):
        """C2 of the input (the first residual stage's output) as a new padded-tap tensor, ring-padded NHWC fp16 [n,162,162,c] with c = 64
        (ResNet-18) or 256 (ResNet-50): forward_trunk(x)[0]'s bits, but only the stem and that stage run (include/vtd.h
        vtd_detector_forward_c2).  Needs options fuse_fpn_head=0."""
        with self.lock:
            n, keep = self._set_input(x)
            tap = torch.empty((n, 162, 162, 256 if self.backbone == "resnet50" else 64), dtype=torch.float16, device="cuda")
            _native.check(self.lib.vtd_detector_forward_c2(self.handle, n, C.c_void_p(tap.data_ptr()), _stream_ptr()),
                          "vtd_detector_forward_c2")
            del keep
            return tap

    def read_tap(self, name, n):
        shapes = {"input": (3, 640, 640), "stem": (64, 320, 320), "pool": (64, 160, 160), "p2": (256, 160, 160), "head1": (64, 160, 160),
                  "head2": (64, 320, 320)}
        if name not in shapes:
            wide = self.backbone == "resnet50"
            idx = int(name[1]) - 2
            ch = (64, 128, 256, 512)[idx] * (4 if wide else 1)
            shapes[name] = (ch, 160 >> idx, 160 >> idx)
        c, h, w = shapes[name]
        out = np.empty((n, c, h, w), np.float32)
        with self.lock:
            _native.check(self.lib.vtd_detector_read_tap(self.handle, name.encode(), n, out.ctypes.data, out.size, _stream_ptr()),
                          f"vtd_detector_read_tap({name})")
        return out


class PostProcessor:
    """``TextDetector._post_process`` on the GPU for a batch of probability maps (vtd_postproc_*)."""

    def __init__(self, max_batch, map_h=640, map_w=640, max_out=1024):
        self.lib = _native.require()
        self.max_batch, self.h, self.w, self.max_out = max_batch, map_h, map_w, max_out
        self.lock = threading.Lock()
        h = C.c_void_p()
        _native.check(self.lib.vtd_postproc_create(max_batch, map_h, map_w, max_out, C.byref(h)), "vtd_postproc_create")
        self.handle = h
        self.records = torch.empty((max_batch, max_out, 16), dtype=torch.int32, device="cuda")
        self.counts = torch.empty((max_batch,), dtype=torch.int32, device="cuda")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vtd_postproc_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_device(self, prob, orig_w, orig_h, threshold, records=None, counts=None):
        """Enqueue only; returns (records[n,max_out,16] int32 view, counts[n]) device tensors.  Pass `records` /
        `counts` to keep several batches in flight (the default buffers are overwritten by the next call)."""
        n = prob.shape[0]
        records = self.records if records is None else records
        counts = self.counts if counts is None else counts
        if prob.dtype != torch.float32 or not prob.is_cuda or tuple(prob.shape[-2:]) != (self.h, self.w):
            raise ValueError("probability maps must be float32 cuda tensors of the workspace's map size")
        prob = prob.reshape(n, self.h, self.w).contiguous()
        ow = np.ascontiguousarray(orig_w, dtype=np.int32)
        oh = np.ascontiguousarray(orig_h, dtype=np.int32)
        _native.check(self.lib.vtd_postproc_run(self.handle, C.c_void_p(prob.data_ptr()), n, ow.ctypes.data, oh.ctypes.data,
                                                float(threshold), C.c_void_p(records.data_ptr()),
                                                C.c_void_p(counts.data_ptr()), _stream_ptr()), "vtd_postproc_run")
        self._keep = (prob, ow, oh)
        return records[:n], counts[:n]

    def run(self, prob, orig_w, orig_h, threshold, debug=False):
        with self.lock:
            rec, cnt = self.run_device(prob, orig_w, orig_h, threshold)
            cnt = cnt.cpu().numpy()
            if int(cnt.max(initial=0)) > self.max_out:
                import logging
                logging.getLogger(__name__).warning(f"frame with {int(cnt.max())} components exceeds max_detections={self.max_out}; "
                                                    "extra detections dropped")
            kmax = int(min(cnt.max(initial=0), self.max_out))
            rec = rec[:, :kmax].cpu().numpy() if kmax else np.zeros((len(cnt), 0, 16), np.int32)
        return [records_to_dicts(rec[i, :min(int(cnt[i]), self.max_out)], debug) for i in range(len(cnt))]


def records_to_dicts(rec, debug=False):
    """vtd_detection records -> the reference's detection dicts (text_detector.py:172-176): plain Python ints/floats."""
    if len(rec) == 0:
        return []
    bbox = rec[:, 0:4].tolist()
    poly = rec[:, 4:12].reshape(-1, 4, 2).tolist()
    conf = np.ascontiguousarray(rec[:, 12]).view(np.float32).tolist()
    out = [{"bbox": b, "confidence": c, "polygon": p} for b, c, p in zip(bbox, conf, poly)]
    if debug:
        area = np.ascontiguousarray(rec[:, 13]).view(np.float32).tolist()
        first = rec[:, 14:16].tolist()
        for d, a, f in zip(out, area, first):
            d["_area"] = a
            d["_first"] = tuple(f)
    return out


def detector_profile(engine):
    """[(description, total_ms, calls, total_macs)] per launch slot of a DetectorEngine (after set_profiling(1))."""
    lib, out = engine.lib, []
    name = C.create_string_buffer(160)
    ms, calls, macs = C.c_double(), C.c_int64(), C.c_double()
    for i in range(lib.vtd_detector_num_ops(engine.handle)):
        _native.check(lib.vtd_detector_get_profile(engine.handle, i, name, 160, C.byref(ms), C.byref(calls), C.byref(macs),
                                                   _stream_ptr()), "vtd_detector_get_profile")
        out.append((name.value.decode(), ms.value, calls.value, macs.value))
    return out


class RecognizerEngine(_Tunable):
    """CRNN on the GPU: crops (or reference-format [n,3,32,128] tensors) in, [n,31,V] logits / decoded text out."""

    _kind = "recognizer"

    T = 31

    def __init__(self, vocab_size, state_dict, max_crops=None, options=None):
        self.lib = _native.require()
        self.vocab_size = vocab_size
        self.max_crops = max_crops or int(os.environ.get("VTD_MAX_CROPS", "512"))
        self.lock = threading.Lock()
        h = C.c_void_p()
        _native.check(self.lib.vtd_recognizer_create(vocab_size, self.max_crops, C.byref(h)), "vtd_recognizer_create")
        self.handle = h
        try:
            # VTD_RECOGNIZER_OPTIONS="fuse_pools=0": build options for A/B measurements (include/vtd.h: vtd_recognizer_set_option)
            env_opts = {k: int(v) for k, v in (kv.split("=") for kv in os.environ.get("VTD_RECOGNIZER_OPTIONS", "").split(",") if kv)}
            for name, value in {**env_opts, **(options or {})}.items():
                _native.check(self.lib.vtd_recognizer_set_option(h, name.encode(), int(value)), f"vtd_recognizer_set_option({name})")
            for key, value in state_dict.items():
                if key.endswith("num_batches_tracked"):
                    continue
                arr = np.ascontiguousarray(value.detach().cpu().float().numpy())
                _native.check(self.lib.vtd_recognizer_set_tensor(h, key.encode(), arr.ctypes.data, arr.size),
                              f"vtd_recognizer_set_tensor({key})")
            _native.check(self.lib.vtd_recognizer_finalize(h, _stream_ptr()), "vtd_recognizer_finalize")
            self.set_tuning(shipped_tuning_text())
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vtd_recognizer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def macs_per_crop(self):
        return int(self.lib.vtd_recognizer_macs_per_crop(self.handle))

    def _forward_current(self, n):
        logits = torch.empty((n, self.T, self.vocab_size), dtype=torch.float32, device="cuda")
        _native.check(self.lib.vtd_recognizer_forward(self.handle, n, C.c_void_p(logits.data_ptr()), _stream_ptr()),
                      "vtd_recognizer_forward")
        return logits

    def forward_logits(self, x):
        """CRNN.forward on a reference-format tensor [n,3,32,128] (any device) -> [n,31,V] f32 cuda."""
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (3, 32, 128):
            raise ValueError("CRNN input must be [n,3,32,128] float")
        outs = []
        with self.lock:
            for i in range(0, x.shape[0], self.max_crops):
                xd = x[i:i + self.max_crops].to("cuda", torch.float32).contiguous()
                _native.check(self.lib.vtd_recognizer_set_input_nchw(self.handle, C.c_void_p(xd.data_ptr()), xd.shape[0], _stream_ptr()),
                              "vtd_recognizer_set_input_nchw")
                outs.append(self._forward_current(xd.shape[0]))
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def load_crops(self, frames, boxes):
        """K6 + conv1 for boxes [(frame, x1, y1, x2, y2), ...] on a DeviceFrames batch; call with the lock held."""
        b = boxes if torch.is_tensor(boxes) else torch.as_tensor(np.asarray(boxes, dtype=np.int32).reshape(-1, 5))
        b = b.to("cuda", torch.int32).contiguous()
        n = b.shape[0]
        frames.wait_ready()
        _native.check(self.lib.vtd_recognizer_crop_resize(self.handle, C.c_void_p(frames.tensor.data_ptr()), frames.n, frames.height,
                                                          frames.width, C.c_void_p(b.data_ptr()), n, _stream_ptr()),
                      "vtd_recognizer_crop_resize")
        self._keep = (b, frames)
        return n

    def forward_crops(self, frames, boxes):
        with self.lock:
            n = self.load_crops(frames, boxes)
            return self._forward_current(n)

    def submit_decode(self, frames, boxes_np, id2char_dev, blank_id=0):
        """Enqueue crop/resize -> CRNN -> softmax+CTC decode for boxes_np ([k,5] int32) and an asynchronous copy of the
        decoded records to pinned host memory.  Returns a ticket for ``finish_decode`` (nothing synchronises here)."""
        k = int(boxes_np.shape[0])
        host_boxes = PINNED.take((k, 5))
        host_boxes.numpy()[...] = boxes_np
        with self.lock:
            dev_boxes = host_boxes.to("cuda", non_blocking=True)
            n = self.load_crops(frames, dev_boxes)
            logits = self._forward_current(n)
            out = torch.empty((k, 2 + self.T), dtype=torch.int32, device="cuda")
            _native.check(self.lib.vtd_ctc_greedy_decode(C.c_void_p(logits.data_ptr()), k, self.T, self.vocab_size,
                                                         C.c_void_p(id2char_dev.data_ptr()), blank_id, 1, C.c_void_p(out.data_ptr()),
                                                         _stream_ptr()), "vtd_ctc_greedy_decode")
            host = PINNED.take((k, 2 + self.T))
            copy_to_pinned(host, out)
            ev = torch.cuda.Event()
            ev.record()
        return {"host": host, "event": ev, "keep": (host_boxes, dev_boxes, logits, out, frames)}

    @staticmethod
    def finish_decode(ticket):
        ticket["event"].synchronize()
        out = decode_records_to_text(ticket["host"].numpy())
        PINNED.release(ticket["host"], ticket["event"])
        PINNED.release(ticket["keep"][0], ticket["event"])
        return out

    TAP_SHAPES = {"resized": (32, 128, 3), "conv1": (64, 16, 64), "conv2": (128, 8, 32), "conv3": (256, 8, 32), "conv4": (256, 4, 32),
                  "conv5": (512, 4, 32), "conv6": (512, 2, 32), "cnn": (512, 1, 31), "h0": (512, 1, 31), "h1": (512, 1, 31)}

    def read_tap(self, name, n):
        shape = (n,) + self.TAP_SHAPES.get(name, (512, 1, 31))   # an unknown name is the library's error to raise
        out = np.empty(shape, np.float32)
        with self.lock:
            _native.check(self.lib.vtd_recognizer_read_tap(self.handle, name.encode(), n, out.ctypes.data, out.size, _stream_ptr()),
                          f"vtd_recognizer_read_tap({name})")
        return out


def ctc_greedy_decode(logits, id2char, blank_id=0, apply_softmax=True):
    """[softmax +] the reference's greedy decode on the GPU.  logits: [n,T,V] float tensor (any device), logits when
    apply_softmax else probabilities; id2char: list of code points / -1.  Returns [(text, confidence)]."""
    lib = _native.require()
    lg = logits.detach().to("cuda", torch.float32).contiguous()
    n, T, V = lg.shape
    table = torch.tensor(list(id2char)[:V] + [-1] * max(0, V - len(id2char)), dtype=torch.int32, device="cuda")
    out = torch.empty((n, 2 + T), dtype=torch.int32, device="cuda")
    _native.check(lib.vtd_ctc_greedy_decode(C.c_void_p(lg.data_ptr()), n, T, V, C.c_void_p(table.data_ptr()), blank_id,
                                            1 if apply_softmax else 0, C.c_void_p(out.data_ptr()), _stream_ptr()),
                  "vtd_ctc_greedy_decode")
    return decode_records_to_text(out.cpu().numpy())


def decode_records_to_text(host):
    """[n][2+T] int32 decode records -> [(text, confidence)]."""
    conf = np.ascontiguousarray(host[:, 1]).view(np.float32).tolist()
    lens = host[:, 0].tolist()
    rows = host[:, 2:].tolist()
    return [("".join(map(chr, rows[i][:lens[i]])), conf[i]) for i in range(len(lens))]


def plan_passes(rows, pass_tickets, max_crops):
    """The recogniser passes of queued tickets with `rows[i]` crops each: groups of `pass_tickets` consecutive tickets, every group cut
    into passes of at most `max_crops` rows.  A pass is a list of runs (ticket index, first row, rows, offset in the pass), one per
    stretch of consecutive rows of one ticket -- one staging launch each."""
    passes = []
    for g in range(0, len(rows), pass_tickets):
        runs, used = [], 0
        for i in range(g, min(g + pass_tickets, len(rows))):
            first = 0
            while first < rows[i]:
                if used == max_crops:
                    passes.append(runs)
                    runs, used = [], 0
                n = min(rows[i] - first, max_crops - used)
                runs.append((i, first, n, used))
                first += n
                used += n
        if runs:
            passes.append(runs)
    return passes


class TrOCREngine(_Tunable):
    """The Transformer recogniser on the GPU (include/vtd.h: vtd_trocr_*): crops of resident frames, or the
    ``pixel_values`` tensor the reference hands to ``generate``, in; greedy token ids out."""

    _kind = "trocr"

    def __init__(self, spec, state_dict, max_crops=None, slots=None, xattn=None):
        from .trocr_spec import hf4_key
        self.lib = _native.require()
        self.spec = spec
        self.max_crops = max_crops or int(os.environ.get("VTD_TROCR_MAX_CROPS", "256"))   # rows per encoder pass / decode (~20 MB of HBM each:
                                                                                            # workspaces + caches + a 0.89 MB slot; 47 MB with the 28 MB slot of xattn=False)
        self.lock = threading.Lock()
        cfg = _native.TrocrConfig(spec.image_size, spec.patch_size, spec.enc_hidden, spec.enc_layers, spec.enc_heads, spec.enc_ffn,
                                  int(spec.enc_qkv_bias), spec.enc_ln_eps, spec.dec_hidden, spec.dec_layers, spec.dec_heads, spec.dec_ffn,
                                  spec.vocab_size, spec.max_positions, spec.dec_ln_eps, spec.decoder_start_token_id, spec.eos_token_id,
                                  spec.pad_token_id, spec.max_length)
        h = C.c_void_p()
        _native.check(self.lib.vtd_trocr_create(C.byref(cfg), self.max_crops, C.byref(h)), "vtd_trocr_create")
        self.handle = h
        try:
            # one encoder-output slot unless a caller asks for the second one
            _native.check(self.lib.vtd_trocr_set_option(h, b"slots", int(slots or 1)), "vtd_trocr_set_option(slots)")
            # decoder cross-attention on the raw encoder states (csrc/trocr_xattn.hip; include/vtd.h option "xattn") unless asked for the
            # reference's per-layer key / value projections: xattn=False, or VTD_TROCR_XATTN=0
            want_xattn = (os.environ.get("VTD_TROCR_XATTN", "1") != "0") if xattn is None else bool(xattn)
            _native.check(self.lib.vtd_trocr_set_option(h, b"xattn", int(want_xattn)), "vtd_trocr_set_option(xattn)")
            for key, value in state_dict.items():
                arr = np.ascontiguousarray(value.detach().cpu().float().numpy())
                _native.check(self.lib.vtd_trocr_set_tensor(h, hf4_key(key).encode(), arr.ctypes.data, arr.size), f"vtd_trocr_set_tensor({key})")
            _native.check(self.lib.vtd_trocr_finalize(h, _stream_ptr()), "vtd_trocr_finalize")
            self.set_tuning(shipped_tuning_text())
        except Exception:
            self.close()
            raise
        self.tokens = int(self.lib.vtd_trocr_encoder_tokens(h))
        self.logits_stride = int(self.lib.vtd_trocr_logits_stride(h))
        self.slots = int(self.lib.vtd_trocr_num_slots(h))
        form = C.c_int()
        _native.check(self.lib.vtd_trocr_get_option(h, b"xattn", C.byref(form)), "vtd_trocr_get_option(xattn)")
        self.xattn = bool(form.value)   # the form that runs (a geometry the kernel does not cover keeps the key / value form)
        self._next_slot = 0
        self._setup_passes()

    def close(self):
        """Stops the worker thread, then destroys the handle -- unless the worker is still inside a pass: the handle is then left
        alive (leaked) rather than destroyed under it."""
        worker = None
        if getattr(self, "_qlock", None) is not None:
            with self._qlock:   # submit_crops raises from here on; jobs the worker has not started are dropped
                self._closed = True
                self._generation += 1
                worker = self._worker
                if worker is not None:
                    self._jobs.put(None)
        if worker is not None and worker.is_alive():
            if sys.is_finalizing():   # (a daemon thread may be frozen anywhere at exit)
                return
            worker.join(timeout=60)
            if worker.is_alive():
                logger.error("TrOCREngine.close: the recogniser worker is still inside a pass after 60 s; its handle is left alive")
                return
        if getattr(self, "handle", None):
            with self.lock:
                if not sys.is_finalizing():   # passes may still run on the streams their tickets came from
                    try:
                        torch.cuda.synchronize()
                    except Exception:
                        pass
                self.lib.vtd_trocr_destroy(self.handle)
                self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def macs_per_crop(self):
        return int(self.lib.vtd_trocr_macs_per_crop(self.handle))

    @property
    def last_steps(self):
        """Decoder steps the last generate call enqueued (it stops once every row has emitted </s>)."""
        return int(self.lib.vtd_trocr_last_steps(self.handle))

    def encode_pixels(self, pixel_values, slot=0):
        """[n,3,S,S] float (any device): ViT encoder + cross-attention keys / values into `slot`.  Call with the lock held."""
        s = self.spec.image_size
        if not torch.is_tensor(pixel_values) or pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, s, s):
            raise ValueError(f"pixel_values must be [n,3,{s},{s}] float")
        x = pixel_values.to("cuda", torch.float32).contiguous()
        _native.check(self.lib.vtd_trocr_encode_pixels_slot(self.handle, slot, C.c_void_p(x.data_ptr()), x.shape[0], _stream_ptr()),
                      "vtd_trocr_encode_pixels")
        self._keep = x
        return x.shape[0]

    def encode_crops(self, frames, boxes, slot=0):
        """boxes [(frame, x1, y1, x2, y2), ...] of a DeviceFrames batch into `slot`.  Call with the lock held."""
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 5))
        frames.wait_ready()
        _native.check(self.lib.vtd_trocr_encode_crops_slot(self.handle, slot, C.c_void_p(frames.tensor.data_ptr()), frames.n, frames.height,
                                                           frames.width, b.ctypes.data, b.shape[0], _stream_ptr()), "vtd_trocr_encode_crops")
        self._keep = (b, frames)
        return b.shape[0]

    def _enqueue_generate(self, n, slot, max_length=None, forced=None, want_logits=False):
        """Greedy decode of the n crops encoded into `slot`, on the CURRENT stream.  Returns device tensors (ids, logits | None); the
        call itself returns once all but the last two decoder steps have run (the handle paces itself two steps behind the GPU)."""
        max_length = max_length or self.spec.max_length
        ids = torch.empty((n, max_length), dtype=torch.int32, device="cuda")
        logits = torch.zeros((n, max_length - 1, self.logits_stride), dtype=torch.float32, device="cuda") if want_logits else None
        fdev, flen = None, 0
        if forced is not None:
            fdev = torch.as_tensor(np.asarray(forced), dtype=torch.int32).to("cuda").contiguous()
            flen = fdev.shape[1]
        _native.check(self.lib.vtd_trocr_generate_slot(self.handle, slot, n, max_length, C.c_void_p(fdev.data_ptr()) if fdev is not None else None,
                                                       flen, C.c_void_p(ids.data_ptr()), C.c_void_p(logits.data_ptr()) if logits is not None else None,
                                                       _stream_ptr()), "vtd_trocr_generate")
        self._keep_gen = (fdev,)
        return ids, logits

    def generate_current(self, n, max_length=None, forced=None, want_logits=False, slot=0):
        """Greedy decode of the n crops encoded last into `slot`.  Returns (ids [n,max_length] int32 cpu tensor, logits or None)."""
        ids, logits = self._enqueue_generate(n, slot, max_length, forced, want_logits)
        out = ids.cpu()
        return out, (logits[..., :self.spec.vocab_size].cpu() if logits is not None else None)

    def generate_pixels(self, pixel_values, **kw):
        outs = []
        with self.lock:
            for i in range(0, pixel_values.shape[0], self.max_crops):
                n = self.encode_pixels(pixel_values[i:i + self.max_crops])
                outs.append(self.generate_current(n, **kw))
        ids = torch.cat([o[0] for o in outs])
        logits = torch.cat([o[1] for o in outs]) if outs[0][1] is not None else None
        return ids, logits

    def generate_crops(self, frames, boxes, **kw):
        outs = []
        with self.lock:
            for i in range(0, len(boxes), self.max_crops):
                n = self.encode_crops(frames, boxes[i:i + self.max_crops])
                outs.append(self.generate_current(n, **kw)[0])
        return torch.cat(outs)

    # ---- pipelined use: recogniser batches are decoupled from detector batches ---------------------------------------------------
    # A decode step costs about the same whether 30 or 300 rows are live (~136 dependent launches), so crops are worth collecting:
    # submit_crops only QUEUES a ticket; the GPU work starts when some ticket's result is asked for (finish) or the queue would
    # overflow the workspace.  Queued tickets are then cut into PASSES (plan_passes) of `pass_tickets` tickets (VTD_TROCR_PASS_TICKETS,
    # default 2); every pass is ONE encoder pass into an encoder-output slot and ONE decode right behind it, on the same stream.
    #
    # A caller keeps `pipeline_lag` = pass_tickets - 1 tickets in flight behind the one it asks for (VideoTextPipeline._pipeline_push and
    # bench.py do), so that a whole pass is queued when its first ticket is finished; with fewer in flight the passes are simply smaller.
    #
    # Asynchronous passes (VTD_TROCR_ASYNC=1): a full pass (pass_tickets tickets) goes to a worker thread, which stages, encodes and
    # decodes it while the submitting thread keeps feeding the detector -- a pass blocks its host thread for its whole (host-paced)
    # decode, during which the caller's thread otherwise submits nothing: the detector's launches of the next pass's batches then fall
    # into the decode's launch-bound tail instead of running while the recogniser's streams sit idle.  The caller keeps two passes of
    # tickets in flight (pipeline_lag = 2 pass_tickets - 1).
    def _setup_passes(self):
        self.pass_tickets = max(1, int(os.environ.get("VTD_TROCR_PASS_TICKETS", "2")))
        self.async_passes = os.environ.get("VTD_TROCR_ASYNC", "0") == "1"
        self.pipeline_lag = 2 * self.pass_tickets - 1 if self.async_passes else max(1, self.pass_tickets - 1)
        self._queue = []          # tickets whose crops are not staged yet (submit_crops / finish)
        self._qlock = threading.Lock()   # the queue, the worker and the generation: submitting never waits for a pass
        self._jobs = queue.Queue()
        self._worker = None
        self._generation = 0      # bumped by discard_queue / close: jobs of an older generation are dropped by the worker
        self._closed = False

    def submit_crops(self, frames, boxes):
        """Queue the crops `boxes` ([(frame, x1, y1, x2, y2), ...]) of a resident frame batch; returns a ticket for ``finish``.  Nothing
        is enqueued on the GPU unless the queue has to be flushed to make room (VTD_TROCR_MERGE=0: every ticket runs on its own,
        at once)."""
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 5))
        ticket = {"boxes": b, "frames": frames, "stream": torch.cuda.current_stream(), "parts": None}
        merge = os.environ.get("VTD_TROCR_MERGE", "1") != "0"
        if self.async_passes and merge:
            with self._qlock:
                self._check_open()
                self._queue.append(ticket)
                if len(self._queue) >= self.pass_tickets:
                    group, self._queue = self._queue[:self.pass_tickets], self._queue[self.pass_tickets:]
                    for t in group:
                        t["ready"] = threading.Event()
                    if self._worker is None:
                        self._worker = threading.Thread(target=self._worker_loop, name="vtd-trocr-pass", daemon=True)
                        self._worker.start()
                    self._jobs.put((self._generation, group, torch.cuda.current_device()))
            return ticket
        with self.lock:
            self._check_open()
            if sum(len(t["boxes"]) for t in self._queue) + len(b) > self.max_crops:
                self._flush()
            with self._qlock:
                self._queue.append(ticket)
            if not merge:
                self._flush()
        return ticket

    def _check_open(self):
        if self._closed:
            raise _native.NativeError("TrOCREngine is closed")

    def _worker_loop(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            generation, group, device = job
            try:
                torch.cuda.set_device(device)
                with self.lock:
                    if generation == self._generation:
                        self._run_tickets(group, len(group))
            except Exception as e:   # finish() reports it per ticket (parts stay None), as for a synchronous pass that raised
                logger.error(f"TrOCREngine: recogniser pass failed: {e}")
            finally:
                for t in group:
                    t["ready"].set()

    def _flush(self):
        """Everything queued runs now, in passes (lock held)."""
        with self._qlock:
            tickets, self._queue = self._queue, []
        self._run_tickets(tickets, self.pass_tickets if os.environ.get("VTD_TROCR_MERGE", "1") != "0" else 1)

    def _run_tickets(self, tickets, pass_tickets):
        """Every pass of `tickets` (lock held).  Only once all of them were enqueued do the tickets get their `parts`, a list of
        (pass, first row, rows, offset in the pass): an exception leaves every ticket without parts (finish reports the failure)."""
        done = []
        try:
            for runs in plan_passes([len(t["boxes"]) for t in tickets], pass_tickets, self.max_crops):
                done.append((self._run_pass(tickets, runs), runs))
        except Exception:
            for pas, _ in done:
                PINNED.release(pas["host"], pas["event"])
            raise
        for t in tickets:
            t["parts"] = []   # (a ticket keeps its frames until it is finished: the staging launches read them asynchronously)
        for pas, runs in done:
            pas["users"] = len(runs)
            for i, first, n, off in runs:
                tickets[i]["parts"].append((pas, first, n, off))

    def _run_pass(self, tickets, runs):
        """One planned pass (lock held), on the stream its last ticket was submitted from: stage every run into the next slot, encode,
        decode (host-paced: returns when all but the last two decoder steps have run), copy the ids to a pinned buffer and record the
        event that guards it.  Returns the pass {"host", "event"}."""
        slot = self._next_slot
        self._next_slot = (slot + 1) % self.slots
        with torch.cuda.stream(tickets[runs[-1][0]]["stream"]):
            for i, first, n, off in runs:
                fr = tickets[i]["frames"]
                fr.wait_ready()
                bb = np.ascontiguousarray(tickets[i]["boxes"][first:first + n])
                _native.check(self.lib.vtd_trocr_stage_crops_slot(self.handle, slot, C.c_void_p(fr.tensor.data_ptr()), fr.n, fr.height, fr.width,
                                                                  bb.ctypes.data, n, off, _stream_ptr()), "vtd_trocr_stage_crops")
            rows = runs[-1][3] + runs[-1][2]
            _native.check(self.lib.vtd_trocr_encode_staged_slot(self.handle, slot, rows, _stream_ptr()), "vtd_trocr_encode_staged")
            ids, _ = self._enqueue_generate(rows, slot)
            host, event = PINNED.take(tuple(ids.shape)), torch.cuda.Event()
            try:
                copy_to_pinned(host, ids)
                event.record()
            except Exception:
                event.record()   # behind whatever of the copy was enqueued
                PINNED.release(host, event)
                raise
        return {"host": host, "event": event}

    def finish(self, ticket):
        """ids [n, max_length] int32 (cpu) of a ticket, rows in the order of its boxes.  Flushes the queue when the ticket is still in
        it.  Host-blocking: returns when this ticket's decodes have finished."""
        if ticket["parts"] is None and "ready" not in ticket:
            with self.lock:
                if ticket["parts"] is None:
                    self._flush()
        if "ready" in ticket:
            ticket["ready"].wait()     # its pass runs (or ran) on the worker thread
        if ticket["parts"] is None:    # its pass raised half way (the exception went to whoever triggered the flush)
            raise _native.NativeError("the recogniser pass this ticket was queued for failed")
        out = torch.empty((len(ticket["boxes"]), self.spec.max_length), dtype=torch.int32)
        try:
            for pas, first, n, off in ticket["parts"]:
                pas["event"].synchronize()
                out[first:first + n] = pas["host"][off:off + n]
        finally:
            for pas, *_ in ticket["parts"]:
                pas["users"] -= 1
                if pas["users"] == 0:
                    PINNED.release(pas.pop("host"), pas["event"])
            ticket["parts"] = []
            ticket["frames"] = None
        return out

    def discard_queue(self):
        """Drop every ticket that has not been finished (an abandoned video): queued tickets release their frame batches, jobs the worker
        has not started are dropped, and the device is synchronised so that no pass still writes a pinned buffer once its tickets go."""
        with self.lock:
            with self._qlock:
                self._generation += 1
                for t in self._queue:
                    t["frames"] = None
                    t["parts"] = None
                self._queue = []
            torch.cuda.synchronize()

    def set_profiling(self, mode):
        _native.check(self.lib.vtd_trocr_set_profiling(self.handle, int(mode)), "vtd_trocr_set_profiling")

    def profile(self):
        """(total ms, launches, summed row counts) of the bracketed cross-attention launches since the last call."""
        ms, calls, rows = C.c_double(), C.c_int64(), C.c_int64()
        torch.cuda.synchronize()
        _native.check(self.lib.vtd_trocr_get_profile(self.handle, C.byref(ms), C.byref(calls), C.byref(rows), _stream_ptr()),
                      "vtd_trocr_get_profile")
        return ms.value, calls.value, rows.value

    def gemm_profile(self):
        """(total ms, launches, executed FLOPs) of the encoder pass's dense-GEMM launches bracketed since the last call (profiling mode bit 1)."""
        ms, calls, flops = C.c_double(), C.c_int64(), C.c_double()
        torch.cuda.synchronize()
        _native.check(self.lib.vtd_trocr_get_gemm_profile(self.handle, C.byref(ms), C.byref(calls), C.byref(flops), _stream_ptr()),
                      "vtd_trocr_get_gemm_profile")
        return ms.value, calls.value, flops.value

    def read_tap(self, name, n):
        s = self.spec
        shape = (n, 3, s.image_size, s.image_size) if name == "pixel_values" else (n, self.tokens, s.enc_hidden)
        out = np.empty(shape, np.float32)
        with self.lock:
            _native.check(self.lib.vtd_trocr_read_tap(self.handle, name.encode(), n, out.ctypes.data, out.size, _stream_ptr()),
                          f"vtd_trocr_read_tap({name})")
        return out


def trim_generated(ids, spec):
    """Rows of generate()'s id matrix -> lists cut after <eos> (the start token, which is also id 2, stays)."""
    out = []
    for row in ids.tolist():
        seq = [row[0]]
        for tok in row[1:]:
            seq.append(tok)
            if tok == spec.eos_token_id:
                break
        while len(seq) > 1 and seq[-1] == spec.pad_token_id:
            seq.pop()
        out.append(seq)
    return out
