"""Audio-only inference: the trained student alone, from eight microphone waveforms (or their ready-made spectrogram stack) to boxes.

What the reference's evaluation does with the student (get_predictions_multiteacher, src/utils/utils.py:1720-1830: eval-mode forward,
EfficientDet_post_processing, logits_to_ground_truth) WITHOUT the three teachers it runs beside it: one frozen `Net` through the
folded-BatchNorm kernels, the post-processing kernels the distillation step uses for its pseudo-labels (`postproc.decode_nms`), and
the waveform front end (`audio.MelFrontEnd`, dB maps: the student's stored input is power_to_db of each microphone's mel spectrogram,
mp3_to_pkl.py:31-41).  No teacher, no optimizer state, no gradient arena.

After the first call for an input shape the whole chain - front end, forward, decode, NMS - is one captured hipGraph replayed on
static input buffers, as `DistillEngine.capture` / `replay` do for the training step; a new shape captures anew.

`detect_stream` slides that chain over one long recording that stays on the device: the front end reads the overlapping windows straight
out of it (`mmd_melspec_windows`), a device-side record collects every group's rows (`mmd_det_record_append`, csrc/stream.hip), and the
host synchronises and copies once, at the end.  `track_stream` is the same stream with a tracker (`mmd_track_update`, csrc/track.hip) in
front of every group's append: each row of the record also gets the id of its track."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .arch import NetSpec
from . import _lib
from .audio import MelFrontEnd, stream_window_starts
from .engine import Net
from .postproc import decode_nms, valid_class_mask
from .store import Arena
from . import tracker as _tracker
from .tracker import TrackConfig


class AudioDetector:
    def __init__(self, spec: NetSpec, device, image_size: int = 512, conf_threshold: float = 0.3, nms_threshold: float = 0.5,
                 valid_prediction_ids: Sequence[int] = (6,), label_map: Optional[List[int]] = None, inclusive_nms: bool = False,
                 cand_cap: int = 0, precision: str = "fp32"):
        """The detection settings are the ones `DistillEngine` reads from its StepConfig (`from_step_config`).  cand_cap: rows per image
        of the detection arrays; 0 = every anchor (the reference has no cap), so nothing can overflow."""
        self.device = device
        self.S = int(image_size)
        self.conf_threshold, self.nms_threshold, self.inclusive_nms = float(conf_threshold), float(nms_threshold), bool(inclusive_nms)
        self.net = Net(spec, device, trainable=False, arena=Arena(device, 256 << 20), precision=precision)      # activations only: no tape
        self.front = MelFrontEnd(device)
        self.ws = Arena(device, 64 << 20)         # post-processing workspaces (bump, reset per call)
        lm = label_map if label_map is not None else list(range(spec.num_classes))
        self.label_map = torch.tensor(lm, dtype=torch.int32, device=device)
        self.valid_mask = valid_class_mask(valid_prediction_ids)
        self.cand_cap = int(cand_cap)
        self.cap = int(cand_cap)                  # 0: set to the anchor count at the first call
        self.overflow = torch.zeros(1, dtype=torch.int32, device=device)
        self._graphs: Dict[tuple, dict] = {}      # ("wave", B, N) / ("spec", B, S) -> static input, front-end buffers, graph, outputs
        self.graph_replays = 0                    # calls served by a captured graph
        self.use_graph = True                     # False: every call runs eagerly (timing the graph against the plain launch sequence)
        self._stream: Optional[dict] = None       # detect_stream's buffers and graph: ONE recording at a time (the graph bakes its address in)
        self.stream_captures = 0                  # graphs detect_stream captured
        self.stream_replays = 0                   # groups of windows detect_stream served by a captured graph
        self.last_cls: Optional[torch.Tensor] = None   # head outputs of the last call (views of the net's arena: valid until the next call)
        self.last_reg: Optional[torch.Tensor] = None

    @classmethod
    def from_step_config(cls, spec: NetSpec, device, cfg) -> "AudioDetector":
        """cfg: the `StepConfig` train.py / evaluate.py build from the cfg file (`train.step_config`)."""
        return cls(spec, device, image_size=cfg.image_size, conf_threshold=cfg.conf_threshold, nms_threshold=cfg.nms_threshold,
                   valid_prediction_ids=cfg.valid_prediction_ids, label_map=cfg.label_map, inclusive_nms=cfg.inclusive_nms,
                   cand_cap=cfg.cand_cap, precision=cfg.precision)

    def load(self, state):
        """A student state_dict (a checkpoint's `c["state_dict"]`), as `DistillEngine.load` takes it for the student."""
        self.net.load_state(state)

    # ------------------------------------------------------------------ the chain
    def _buffers(self, kind: str, shape) -> dict:
        """static input (and, for waveforms, the front end's buffers) of one input shape"""
        g = {"x": torch.empty(shape, device=self.device)}
        if kind == "wave":
            B, C, N = shape
            g["mel"] = torch.empty(B, self.front.n_mels, self.front.n_frames(N), C, device=self.device)
            g["max_ws"] = torch.empty(B * C, device=self.device)
            g["audio"] = torch.empty(B, C, self.S, self.S, device=self.device)
        return g

    def _chain(self, kind: str, g: dict):
        """Issues front end -> forward -> decode -> NMS on the current stream; nothing is allocated outside the bump arenas."""
        S = self.S
        if kind == "wave":
            self.front.melspec_into(g["x"], None, True, g["max_ws"], g["mel"])
            audio = self.front.resize_into(g["mel"], S, g["audio"])
        else:
            audio = g["x"]
        self._tail(audio, g)

    def _tail(self, audio: torch.Tensor, g: dict):
        """forward -> decode -> NMS of a ready student input [B, 8, S, S]"""
        S = self.S
        B = audio.shape[0]
        self.ws.reset()
        self.net.begin_step()
        cls, reg, _ = self.net.forward(audio, train=False)
        A = cls.shape[1]
        if self.cap <= 0:
            self.cap = A
        rows, cnt = decode_nms(self.ws, self.net, cls, reg, B, A, S, self.cap, self.conf_threshold, self.valid_mask, self.label_map,
                               self.nms_threshold, self.inclusive_nms, self.overflow)
        g.update(cls=cls, reg=reg, rows=rows, cnt=cnt)

    def _rows(self, g: dict) -> List[np.ndarray]:
        torch.cuda.synchronize()
        self.last_cls, self.last_reg = g["cls"], g["reg"]
        cnt = g["cnt"].cpu().tolist()
        return [g["rows"][i, :cnt[i]].cpu().numpy() for i in range(len(cnt))]

    @torch.no_grad()
    def _detect(self, kind: str, x: torch.Tensor) -> List[np.ndarray]:
        key = (kind,) + tuple(x.shape)
        g = self._graphs.get(key)
        if g is not None and self.use_graph and "graph" in g:
            g["x"].copy_(x, non_blocking=True)
            g["graph"].replay()
            self.graph_replays += 1
            return self._rows(g)
        # no graph for this shape yet: run eagerly on the static buffers (the first run sizes the arenas), then capture
        arenas = (self.ws, self.net.arena, self.net.zarena)
        if g is None:
            for a in arenas:
                a.frozen = False                  # chunks are only ever appended: the graphs of earlier shapes stay valid
            g = self._graphs[key] = self._buffers(kind, tuple(x.shape))
        g["x"].copy_(x, non_blocking=True)
        self._chain(kind, g)
        out = self._rows(g)
        for a in arenas:
            a.frozen = True
        if self.use_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self._chain(kind, g)
            torch.cuda.synchronize()
            g["graph"] = graph
        return out

    def detect_spectrogram(self, audio: torch.Tensor) -> List[np.ndarray]:
        """audio [B, 8, S, S] float32 on the device (dB mel maps resized to the image size: the student's input) -> per image float32
        [n, 6] rows (x1, y1, x2, y2, score, label), the row format `DistillEngine.predict` returns for the student."""
        if audio.dim() != 4 or audio.dtype != torch.float32 or audio.shape[1] != self.net.spec.in_channels or \
                audio.shape[2] != self.S or audio.shape[3] != self.S:
            raise ValueError("detect_spectrogram takes float32 [B, %d, %d, %d]" % (self.net.spec.in_channels, self.S, self.S))
        return self._detect("spec", audio)

    def detect(self, wave: torch.Tensor) -> List[np.ndarray]:
        """wave [B, 8, N] float32 on the device (the microphones' waveforms at 44.1 kHz) -> rows as `detect_spectrogram`, through the
        dB front end: `front.student_input(wave, None, S, db=True)`."""
        if wave.dim() != 3 or wave.dtype != torch.float32 or wave.shape[1] != self.net.spec.in_channels:
            raise ValueError("detect takes float32 [B, %d, N] waveforms" % self.net.spec.in_channels)
        self.front.n_frames(wave.shape[2])        # raises on a waveform too short for the reflect padding
        return self._detect("wave", wave)

    # ------------------------------------------------------------------ streaming
    STREAM_ROWS_PER_WINDOW = 256      # default record size per window when cand_cap = 0 (unlimited rows per image)

    def _stream_chain(self, g: dict):
        """One group of windows: front end on the windows the control row names -> forward -> decode -> NMS [-> track update] -> append
        to the record.  The track update reads the record's count before the append advances it."""
        self.front.melspec_windows_into(g["wave"], g["starts"], g["win_len"], True, g["max_ws"], g["mel"])
        audio = self.front.resize_into(g["mel"], self.S, g["audio"])
        self._tail(audio, g)
        B = audio.shape[0]
        if g["track"] is not None:
            _tracker.update(g["rows"], g["cnt"], g["ctl"], g["rec_state"][0:1], g["rec_cap"], g["rec_track"], g["trk_state"], g["track"])
        _lib.call("mmd_det_record_append", g["rows"], g["cnt"], B, g["rows"].shape[1], g["ctl"], g["rec_rows"], g["rec_win"],
                  g["rec_cap"], g["rec_state"][0:1], g["rec_state"][1:2])

    @torch.no_grad()
    def detect_stream(self, wave: torch.Tensor, win_len: int, hop: int, batch: int = 8, rec_cap: Optional[int] = None):
        """Slides the detector over one recording: wave float32 [8, n_total] on the device -> (rows float32 [R, 6], window int32 [R]),
        numpy arrays: the rows `detect` gives each window, in window order, and the index of each row's window.

        Window w is wave[:, w * hop : w * hop + win_len] for w = 0 .. W-1, W = 1 + (n_total - win_len) // hop
        (`audio.stream_window_starts`); a tail shorter than a full window is DROPPED.  hop is any positive number of samples.  The whole
        recording is resident on the device (8 channels of float32 at 44.1 kHz: 1.4 MB per second); recordings that do not fit are not
        supported.

        The windows run in groups of `batch`; the last, shorter group repeats its last window up to `batch` and only its real windows
        are recorded, so one shape - and one captured graph - serves the recording.  Per group the host queues a device-to-device copy
        of the group's row of a control table (the window starts, the number of real windows, the first window's index; uploaded once
        per call) and the chain front end -> resize -> forward -> decode -> NMS -> record append; nothing waits for the host until the
        last group is queued.  A group's rows have the bits `detect` gives the stack of that group's windows.

        rec_cap: rows the device record holds.  Default: W * cand_cap; with cand_cap = 0 (unlimited rows per image) W *
        STREAM_ROWS_PER_WINDOW (256).  A recording with more rows raises RuntimeError naming the rows needed: pass that as rec_cap.

        The graph bakes in the recording's address: it is kept for (win_len, batch, image size, wave.data_ptr(), n_total) and rec_cap,
        and captured again when any of them changes; the detector holds the buffers of one recording at a time."""
        rows, window, _ = self._run_stream("detect_stream", wave, win_len, hop, batch, rec_cap, None)
        return rows, window

    @torch.no_grad()
    def track_stream(self, wave: torch.Tensor, win_len: int, hop: int, batch: int = 8, rec_cap: Optional[int] = None,
                     track: TrackConfig = TrackConfig()):
        """`detect_stream` with a tracker on the device: -> (rows float32 [R, 6], window int32 [R], track int32 [R]).  rows and window
        have exactly the bits `detect_stream` gives; track[i] is the id of the track row i belongs to - ids start at 0 for every call,
        rise in order of birth and are never reused - or -1 (a row that neither continued nor started a track).

        The rule (`tracker.TrackConfig`, DESIGN.md streaming tracking): per window every live track is moved by its velocity, tracks and
        boxes of equal label are paired greedily by IoU >= iou_min, a paired track takes the box and corrects its velocity by beta of
        the centre's residual, an unpaired track is kept for max_age windows, an unpaired box of score >= birth_score starts a track.

        The chain is detect_stream's with `mmd_track_update` between a group's NMS and its record append, in a captured graph of its
        own: the stream key carries the tracking parameters, so `detect_stream` and `track_stream` never replay each other's graph.
        The tracker's state is zeroed with the record's before the first group; still one synchronisation and one copy at the end.
        More than max_tracks live tracks, or more than 256 boxes in one window, raise RuntimeError."""
        if not isinstance(track, TrackConfig):
            raise ValueError("track_stream: track must be a TrackConfig")
        return self._run_stream("track_stream", wave, win_len, hop, batch, rec_cap, track)

    def _run_stream(self, who: str, wave: torch.Tensor, win_len: int, hop: int, batch: int, rec_cap: Optional[int],
                    track: Optional[TrackConfig]):
        C = self.net.spec.in_channels
        if wave.dim() != 2 or wave.dtype != torch.float32 or wave.shape[0] != C or not wave.is_cuda or not wave.is_contiguous():
            raise ValueError("%s takes one contiguous float32 [%d, n_total] recording on the device" % (who, C))
        win_len, hop, batch, n_total = int(win_len), int(hop), int(batch), int(wave.shape[1])
        if batch < 1 or batch > 1024:
            raise ValueError("%s: batch = %d (1 .. 1024)" % (who, batch))
        starts = stream_window_starts(n_total, win_len, hop)
        W = len(starts)
        if rec_cap is None:
            rec_cap = W * (self.cand_cap if self.cand_cap > 0 else self.STREAM_ROWS_PER_WINDOW)
        rec_cap = int(rec_cap)
        if rec_cap < 1 or rec_cap > 0x7fffffff:
            raise ValueError("%s: rec_cap = %d" % (who, rec_cap))
        # control table, one row per group: int64 starts[batch], then {n_valid, first_window} as two int32 in the last word
        G = (W + batch - 1) // batch
        table = np.empty((G, batch + 1), np.int64)
        tail = table.view(np.int32).reshape(G, 2 * (batch + 1))[:, 2 * batch:]
        for gi in range(G):
            real = starts[gi * batch:(gi + 1) * batch]
            table[gi, :batch] = real + [real[-1]] * (batch - len(real))
            tail[gi] = (len(real), gi * batch)
        table = torch.from_numpy(table).to(self.device)

        key = (win_len, batch, self.S, wave.data_ptr(), n_total, rec_cap, None if track is None else track.key())
        arenas = (self.ws, self.net.arena, self.net.zarena)
        g = self._stream
        if g is None or g["key"] != key:
            self._stream = g = None               # the old recording's buffers go before the new ones come
            for a in arenas:
                a.frozen = False                  # chunks are only ever appended: the graphs of `_detect` stay valid
            cur = torch.zeros(batch + 1, dtype=torch.int64, device=self.device)
            g = {"key": key, "track": track, "wave": wave, "win_len": win_len, "rec_cap": rec_cap, "cur": cur, "starts": cur[:batch],
                 "ctl": cur[batch:].view(torch.int32),
                 "mel": torch.empty(batch, self.front.n_mels, self.front.n_frames(win_len), C, device=self.device),
                 "max_ws": torch.empty(batch * C, device=self.device),
                 "audio": torch.empty(batch, C, self.S, self.S, device=self.device),
                 "rec_rows": torch.empty(rec_cap, 6, device=self.device),
                 "rec_win": torch.empty(rec_cap, dtype=torch.int32, device=self.device),
                 "rec_state": torch.zeros(2, dtype=torch.int32, device=self.device)}       # {rec_count, overflow flag}
            if track is not None:
                g["rec_track"] = torch.empty(rec_cap, dtype=torch.int32, device=self.device)
                g["trk_state"] = _tracker.new_state(self.device, track)
            self._stream = g
        if self.use_graph and "graph" not in g:
            # a warm-up group sizes the arenas (what it appends is dropped: the record's state is zeroed below), then the capture
            g["cur"].copy_(table[0], non_blocking=True)
            self._stream_chain(g)
            torch.cuda.synchronize()
            for a in arenas:
                a.frozen = True
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self._stream_chain(g)
            torch.cuda.synchronize()
            g["graph"] = graph
            self.stream_captures += 1
        g["rec_state"].zero_()
        if track is not None:
            for t in g["trk_state"]:
                t.zero_()
        for gi in range(G):
            g["cur"].copy_(table[gi], non_blocking=True)
            if self.use_graph:
                g["graph"].replay()
                self.stream_replays += 1
            else:
                self._stream_chain(g)
        torch.cuda.synchronize()
        for a in arenas:
            a.frozen = True
        self.last_cls, self.last_reg = g["cls"], g["reg"]
        n, over = g["rec_state"].cpu().tolist()
        self.check_overflow()
        if over or n > rec_cap:
            raise RuntimeError("detection record exceeded: %d rows needed, rec_cap = %d" % (n, rec_cap))
        rows, window = g["rec_rows"][:n].cpu().numpy(), g["rec_win"][:n].cpu().numpy()
        if track is None:
            return rows, window, None
        if int(g["trk_state"][1][1].item()):
            raise RuntimeError(_tracker.overflow_message(track, window))
        return rows, window, g["rec_track"][:n].cpu().numpy()

    def check_overflow(self):
        if int(self.overflow.item()):
            raise RuntimeError("detection capacity exceeded (cand_cap = %d rows per image; 0 = unlimited)" % self.cand_cap)
