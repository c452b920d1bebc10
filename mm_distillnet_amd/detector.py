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
front of every group's append: each row of the record also gets the id of its track.

`open_stream` is the same chain for audio that ARRIVES: a `LiveSession` keeps a bounded ring of samples at a fixed device address
(csrc/live.hip: `mmd_ring_push`, `mmd_ring_push_pcm`), the front end reads the windows out of it across the wrap
(`mmd_melspec_windows_ring`), and one captured graph serves the whole session and every recording pushed through it.  A source at
another rate than 44.1 kHz (`open_stream(sample_rate=R)`) goes through a second ring of input-rate samples, from which
`mmd_ring_resample` computes the 44.1 kHz samples the schedule asks for with the bits `Resampler.resample` gives the whole recording.

`open_bank` is that chain for SEVERAL sources at once: a `LiveBank` keeps one ring and one tracker per session behind one captured
graph, and each row of a group names the session and the window it is (`mmd_melspec_windows_rings`, `mmd_track_update_bank`,
`mmd_det_record_append_bank`), so one forward pass serves one fresh window of every source.  Every session of a bank may have a sample
rate of its own (`open_bank(sample_rates=...)`: an input ring per such session, as `open_stream` keeps one), and `LiveBank.push_all`
sends one round of chunks - one of every session - through one staging copy and one launch each of `mmd_rings_push` and
`mmd_rings_resample`.

A session and a bank differ in their chains - the kernels inside the captured graph, the control row and the record's columns - and in
nothing on the host: a session is the bank's schedule for one session, and `_LiveHost` holds the one path both push through."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .arch import NetSpec
from . import _lib
from .audio import (RINGS_PUSH_DESC, RINGS_RS_DESC, MelFrontEnd, Resampler, bank_reset, bank_round, bank_schedule, bank_state, bank_step,
                    live_group_span, live_in_ring_min, live_pieces, live_resample_ready, resample_ratio, rings_push_entry, rings_push_into,
                    stream_window_starts)
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
        self._graphs: Dict[tuple, SimpleNamespace] = {}     # ("wave", B, N) / ("spec", B, S) -> static input, front-end buffers, graph, outputs
        self.graph_replays = 0                    # calls served by a captured graph
        self.use_graph = True                     # False: every call runs eagerly (timing the graph against the plain launch sequence)
        self._stream: Optional["_GroupChain"] = None      # detect_stream's chain: ONE recording at a time (the graph bakes its address in)
        self.stream_captures = 0                  # graphs detect_stream captured
        self.stream_replays = 0                   # groups of windows detect_stream served by a captured graph
        self._held: Optional["_LiveHost"] = None       # open_stream's session or open_bank's bank; a stream, a session and a bank never coexist
        self.live_captures = 0                    # graphs open_stream's sessions captured
        self.live_replays = 0                     # groups of windows a session served by a captured graph
        self.bank_captures = 0                    # graphs open_bank's banks captured
        self.bank_replays = 0                     # ticks a bank served by a captured graph
        self.resampler: Optional[Resampler] = None     # the filter banks of sessions at other rates than 44.1 kHz (made with the first)
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
    def _buffers(self, kind: str, shape) -> SimpleNamespace:
        """static input (and, for waveforms, the front end's buffers) of one input shape"""
        g = SimpleNamespace(x=torch.empty(shape, device=self.device), graph=None)
        if kind == "wave":
            B, C, N = shape
            g.mel = torch.empty(B, self.front.n_mels, self.front.n_frames(N), C, device=self.device)
            g.max_ws = torch.empty(B * C, device=self.device)
            g.audio = torch.empty(B, C, self.S, self.S, device=self.device)
        return g

    def _chain(self, kind: str, g):
        """Issues front end -> forward -> decode -> NMS on the current stream; nothing is allocated outside the bump arenas."""
        if kind == "wave":
            self.front.melspec_into(g.x, None, True, g.max_ws, g.mel)
            audio = self.front.resize_into(g.mel, self.S, g.audio)
        else:
            audio = g.x
        self._tail(audio, g)

    def _tail(self, audio: torch.Tensor, g):
        """forward -> decode -> NMS of a ready student input [B, 8, S, S]; the outputs become g.cls, g.reg, g.rows, g.cnt"""
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
        g.cls, g.reg, g.rows, g.cnt = cls, reg, rows, cnt

    def _rows(self, g) -> List[np.ndarray]:
        torch.cuda.synchronize()
        self.last_cls, self.last_reg = g.cls, g.reg
        cnt = g.cnt.cpu().tolist()
        return [g.rows[i, :cnt[i]].cpu().numpy() for i in range(len(cnt))]

    def _freeze_arenas(self, frozen: bool):
        """False in front of the first run of a new shape or chain, which sizes the three bump arenas (chunks are only ever appended:
        the graphs captured before stay valid); True behind it, and a graph may be captured"""
        for a in (self.ws, self.net.arena, self.net.zarena):
            a.frozen = frozen

    @staticmethod
    def _capture(issue) -> "torch.cuda.CUDAGraph":
        """the launches of issue() as a graph, on arenas that a run of issue() has sized"""
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            issue()
        torch.cuda.synchronize()
        return graph

    @torch.no_grad()
    def _detect(self, kind: str, x: torch.Tensor) -> List[np.ndarray]:
        key = (kind,) + tuple(x.shape)
        g = self._graphs.get(key)
        if g is not None and self.use_graph and g.graph is not None:
            g.x.copy_(x, non_blocking=True)
            g.graph.replay()
            self.graph_replays += 1
            return self._rows(g)
        # no graph for this shape yet: run eagerly on the static buffers (the first run sizes the arenas), then capture
        if g is None:
            self._freeze_arenas(False)
            g = self._graphs[key] = self._buffers(kind, tuple(x.shape))
        g.x.copy_(x, non_blocking=True)
        self._chain(kind, g)
        out = self._rows(g)
        self._freeze_arenas(True)
        if self.use_graph:
            g.graph = self._capture(lambda: self._chain(kind, g))
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
        self._close_live()                        # one stream, session or bank at a time
        if rec_cap is None:
            rec_cap = W * (self.cand_cap if self.cand_cap > 0 else self.STREAM_ROWS_PER_WINDOW)
        rec_cap = int(rec_cap)
        if rec_cap < 1 or rec_cap > 0x7fffffff:
            raise ValueError("%s: rec_cap = %d" % (who, rec_cap))
        groups = [(starts[first:first + batch], first) for first in range(0, W, batch)]
        table = torch.from_numpy(_GroupChain.control_table(groups, batch)).to(self.device)

        key = (win_len, batch, self.S, wave.data_ptr(), n_total, rec_cap, None if track is None else track.key())
        g = self._stream
        if g is None or g.key != key:
            self._stream = g = None               # the old recording's buffers go before the new ones come
            self._stream = g = _GroupChain(self, "stream", wave, False, win_len, batch, rec_cap, track, key)
            g.prepare()
        g.zero()
        for row in table:
            g.run(row)
        torch.cuda.synchronize()
        self.last_cls, self.last_reg = g.cls, g.reg
        got = g.read(lambda lo, hi: g.blob[lo:hi].cpu().numpy(), int(self.overflow.item()),
                     0 if track is None else int(g.trk_state[1][1].item()))
        return got if track is not None else got + (None,)

    def _overflow_message(self) -> str:
        return "detection capacity exceeded (cand_cap = %d rows per image; 0 = unlimited)" % self.cand_cap

    def check_overflow(self):
        if int(self.overflow.item()):
            raise RuntimeError(self._overflow_message())

    # ------------------------------------------------------------------ live streaming
    @torch.no_grad()
    def open_stream(self, win_len: int, hop: int, batch: int = 8, track: Optional[TrackConfig] = None,
                    ring_len: Optional[int] = None, sample_rate: Optional[int] = None, in_ring_len: Optional[int] = None) -> "LiveSession":
        """Opens a live session: `detect_stream` / `track_stream` (track: a TrackConfig) for audio that arrives in chunks - see
        `LiveSession`.  win_len, hop, batch as `detect_stream`.  ring_len: samples per channel the session keeps on the device, at
        least one group's span (batch - 1) * hop + win_len (ValueError below that); default TWICE that span - the least is the span
        itself, a second one lets a push of up to a span go in as one ring write while the group before it is still pending, and
        the ring stays small against everything else the detector holds (8 channels x 2 x 1.7 s at 44.1 kHz: 4.8 MB for one-second
        windows every 0.1 s in groups of 8).  The detector holds one stream or session at a time: opening one closes the session
        before it and drops `detect_stream`'s buffers, and a later `detect_stream` / `track_stream` closes the session.

        sample_rate: the rate in Hz of the samples that will be pushed.  None or 44100: they are the front end's own, nothing is
        resampled and nothing below exists.  Another rate R: the session resamples to 44.1 kHz as the chunks arrive (`LiveSession`);
        win_len, hop, ring_len and the window indices stay in 44.1 kHz samples.  A ratio `audio.resample_ratio` refuses raises its
        ValueError here.  in_ring_len (only with such a rate): input-rate samples per channel the session keeps, at least
        `audio.live_in_ring_min` (taps + M + 1, and the least span one block of `mmd_ring_resample` stages; ValueError below that);
        default taps + M + ceil(ring_len * M / L) - a push of up to a ring's worth of audio is then one piece."""
        if track is not None and not isinstance(track, TrackConfig):
            raise ValueError("open_stream: track must be a TrackConfig or None")
        self._close_live()
        self._stream = None
        self._held = LiveSession(self, int(win_len), int(hop), int(batch), track, ring_len, sample_rate, in_ring_len)
        return self._held

    def _close_live(self):
        """closes the open session or bank, if any"""
        if self._held is not None:
            self._held.close()

    @torch.no_grad()
    def open_bank(self, n_sessions: int, win_len: int, hop: int, batch: Optional[int] = None, track: Optional[TrackConfig] = None,
                  ring_len: Optional[int] = None, sample_rates: Optional[Sequence] = None, in_ring_len=None) -> "LiveBank":
        """Opens a bank of n_sessions live sessions behind one captured chain - see `LiveBank`: several microphone arrays (or files
        replayed side by side) push independently, and one forward pass serves `batch` ready windows of whichever sessions completed
        them.  win_len, hop, track as `open_stream`; batch: windows per tick, default n_sessions (one fresh window of each);
        ring_len: samples per channel EACH session keeps on the device, at least (batch - 1) * hop + win_len (ValueError below
        that), default twice that.  The detector holds one stream, session or bank at a time: opening any of them closes the others.

        sample_rates: None - every session is pushed 44.1 kHz samples, the default - or one entry per session: None, 44100 or the
        rate in Hz of the samples that session will be pushed.  With None, or no entry other than None / 44100, nothing below exists
        and the bank is the 44.1 kHz bank.  A session at another rate R resamples as its chunks arrive, as `open_stream(sample_rate=R)`
        does (`LiveBank`); win_len, hop, ring_len and the window indices stay in 44.1 kHz samples.  A ratio `audio.resample_ratio`
        refuses raises its ValueError here, before any device work.  in_ring_len (only with such a session): input-rate samples
        per channel that session keeps - one value for all of them, or one entry per session (None where the session is at 44.1
        kHz) - at least `audio.live_in_ring_min`, default taps + M + ceil(ring_len * M / L), both as `open_stream`'s."""
        if track is not None and not isinstance(track, TrackConfig):
            raise ValueError("open_bank: track must be a TrackConfig or None")
        self._close_live()
        self._stream = None
        self._held = LiveBank(self, int(n_sessions), int(win_len), int(hop), int(n_sessions if batch is None else batch), track, ring_len,
                              sample_rates, in_ring_len)
        return self._held


class _GroupChain:
    """The buffers and the graph of one group of `batch` windows, for `detect_stream` / `track_stream` (source: the recording [8,
    n_total]) and for a `LiveSession` (source: its ring [8, ring_len]): front end on the windows the control row names -> resize ->
    forward -> decode -> NMS [-> track update] -> append to the record.

    The control row `cur` is int64 starts[batch], then {n_valid, first_window} as two int32 in the last word (`control_table`).  The
    record is ONE block of int32 words, rows [rec_cap, 6] (float bits) | window [rec_cap] | track [rec_cap] | {count, overflow}, so a
    client may copy it in one piece.

    Third mode, for a `LiveBank` (source: its rings [n_sessions, 8, ring_len]): the rows of a group are windows of several sessions.
    The control row is int64 starts[batch] | int32 sess[batch] | int32 win[batch] | int32 {n_valid, pad} (`bank_control_table`), the
    tracker keeps one state per session, and the record grows by one column: rows | window | track | session | {count, overflow}."""

    COLS = {"stream": 8, "live": 8, "bank": 9}        # int32 words per record row

    def __init__(self, det: AudioDetector, kind: str, source: torch.Tensor, ring: bool, win_len: int, batch: int, rec_cap: int,
                 track: Optional[TrackConfig], key=None):
        dev, C = det.device, det.net.spec.in_channels
        self.det, self.kind, self.source, self.ring, self.win_len, self.rec_cap, self.track, self.key = \
            det, kind, source, ring, win_len, rec_cap, track, key       # kind: "stream" / "live" / "bank", the detector's counters to bump
        self.bank = kind == "bank"
        self.cols = self.COLS[kind]
        self.cur = torch.zeros(2 * batch + 1 if self.bank else batch + 1, dtype=torch.int64, device=dev)
        self.starts, self.ctl = self.cur[:batch], self.cur[-1:].view(torch.int32)
        if self.bank:
            tables = self.cur[batch:2 * batch].view(torch.int32)
            self.sess, self.win = tables[:batch], tables[batch:]
        self.mel = torch.empty(batch, det.front.n_mels, det.front.n_frames(win_len), C, device=dev)
        self.max_ws = torch.empty(batch * C, device=dev)
        self.audio = torch.empty(batch, C, det.S, det.S, device=dev)
        self.blob = blob = torch.zeros(self.cols * rec_cap + 2, dtype=torch.int32, device=dev)
        self.rec_rows = blob[:6 * rec_cap].view(torch.float32).view(rec_cap, 6)
        self.rec_win, self.rec_track, self.rec_state = blob[6 * rec_cap:7 * rec_cap], blob[7 * rec_cap:8 * rec_cap], blob[self.cols * rec_cap:]
        self.trk_state = None if track is None else _tracker.new_state(dev, track)
        if self.bank:
            self.rec_sess = blob[8 * rec_cap:9 * rec_cap]
            self.trk_state = None if track is None else _tracker.new_bank_state(dev, track, source.shape[0])
        self.graph = None

    def issue(self):
        """One group on the current stream.  The track update reads the record's count before the append advances it."""
        det, front = self.det, self.det.front
        if self.bank:
            front.melspec_windows_rings_into(self.source, self.sess, self.starts, self.win_len, True, self.max_ws, self.mel)
        else:
            windows_into = front.melspec_windows_ring_into if self.ring else front.melspec_windows_into
            windows_into(self.source, self.starts, self.win_len, True, self.max_ws, self.mel)
        audio = front.resize_into(self.mel, det.S, self.audio)
        det._tail(audio, self)
        if self.bank:
            if self.track is not None:
                _tracker.update_bank(self.rows, self.cnt, self.ctl, self.sess, self.win, self.rec_state[0:1], self.rec_cap, self.rec_track,
                                     self.trk_state, self.track)
            _lib.call("mmd_det_record_append_bank", self.rows, self.cnt, audio.shape[0], self.rows.shape[1], self.ctl, self.sess, self.win,
                      self.rec_rows, self.rec_win, self.rec_sess, self.rec_cap, self.rec_state[0:1], self.rec_state[1:2])
            return
        if self.track is not None:
            _tracker.update(self.rows, self.cnt, self.ctl, self.rec_state[0:1], self.rec_cap, self.rec_track, self.trk_state, self.track)
        _lib.call("mmd_det_record_append", self.rows, self.cnt, audio.shape[0], self.rows.shape[1], self.ctl, self.rec_rows, self.rec_win,
                  self.rec_cap, self.rec_state[0:1], self.rec_state[1:2])

    def _count(self, what: str):
        """the detector's stream_ / live_ / bank_ captures and replays"""
        setattr(self.det, self.kind + what, getattr(self.det, self.kind + what) + 1)

    def _capture(self):
        self.graph = self.det._capture(self.issue)
        self._count("_captures")

    def prepare(self):
        """A warm-up group sizes the arenas - the control row is still zero: window 0, no real window, nothing recorded or tracked -
        then the capture."""
        det = self.det
        det._freeze_arenas(False)
        self.issue()
        torch.cuda.synchronize()
        det._freeze_arenas(True)
        self.zero()
        if det.use_graph:
            self._capture()

    def run(self, row: torch.Tensor):
        """One group from a control row (device or pinned host memory), replayed or eager"""
        det = self.det
        if det.use_graph and self.graph is None:
            self._capture()                       # prepared with use_graph = False
        self.cur.copy_(row, non_blocking=True)
        if det.use_graph:
            self.graph.replay()
            self._count("_replays")
        else:
            self.issue()

    def zero(self):
        """An empty record, no tracks (ids start at 0 again)"""
        self.rec_state.zero_()
        if self.track is not None:
            for t in self.trk_state:
                t.zero_()

    def zero_tracks(self, s: int):
        """No tracks in session s (its ids start at 0 again), the other sessions' kept; the single-source chain has one session, its
        whole state"""
        if self.track is not None:
            for t in self.trk_state:
                (t[s] if self.bank else t).zero_()

    def read(self, fetch, det_overflow: int, trk_overflow: int):
        """fetch(lo, hi) -> a host copy (numpy int32 the caller does not reuse) of the record's words [lo, hi), made after the
        device finished; the two flags are the detector's and the tracker's overflow -> (rows [n, 6], window [n][, track [n]]); a
        bank's chain: (rows [n, 6], session [n], window [n][, track [n]])"""
        R = self.rec_cap
        n, over = fetch(self.cols * R, self.cols * R + 2).tolist()
        if det_overflow:
            raise RuntimeError(self.det._overflow_message())
        if over or n > R:
            raise RuntimeError("detection record exceeded: %d rows needed, rec_cap = %d" % (n, R))
        rows, window = fetch(0, 6 * n).view(np.float32).reshape(n, 6), fetch(6 * R, 6 * R + n)
        head = (rows, fetch(8 * R, 8 * R + n), window) if self.bank else (rows, window)
        if self.track is None:
            return head
        if trk_overflow:
            raise RuntimeError(_tracker.overflow_message(self.track, window))
        return head + (fetch(7 * R, 7 * R + n),)

    @staticmethod
    def control_table(groups: list, batch: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """groups: (starts [1 .. batch], first_window) per group -> int64 [len(groups), batch + 1], one control row per group: the
        starts, the last one repeated up to batch, then {n_valid, first_window} as two int32 in the last word.  out: an int64
        [>= len(groups), batch + 1] table to write the rows into (a session's pinned one); its first len(groups) rows are returned."""
        table = np.empty((len(groups), batch + 1), np.int64) if out is None else out[:len(groups)]
        tail = table.view(np.int32).reshape(len(groups), 2 * (batch + 1))[:, 2 * batch:]
        for k, (real, first) in enumerate(groups):
            table[k, :batch] = list(real) + [real[-1]] * (batch - len(real))
            tail[k] = (len(real), first)
        return table

    @staticmethod
    def bank_control_table(ticks: list, batch: int, hop: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """ticks: [(session, window), ...] (1 .. batch entries) per tick -> int64 [len(ticks), 2 * batch + 1], one control row per tick of a
        bank's chain: int64 starts[batch] (window * hop) | int32 sess[batch] | int32 win[batch] | int32 {n_valid, 0}, the last real window
        repeated up to batch.  out: an int64 [>= len(ticks), 2 * batch + 1] table to write the rows into; its first len(ticks) rows are
        returned."""
        batch, hop = int(batch), int(hop)
        table = np.empty((len(ticks), 2 * batch + 1), np.int64) if out is None else out[:len(ticks)]
        i32 = table.view(np.int32).reshape(len(ticks), 2 * (2 * batch + 1))
        for k, real in enumerate(ticks):
            if not 1 <= len(real) <= batch:
                raise ValueError(f"a tick of {len(real)} windows at batch = {batch}")
            full = list(real) + [real[-1]] * (batch - len(real))
            table[k, :batch] = [w * hop for _, w in full]
            i32[k, 2 * batch:3 * batch] = [q for q, _ in full]
            i32[k, 3 * batch:4 * batch] = [w for _, w in full]
            i32[k, 4 * batch:] = (len(real), 0)
        return table


def _plan_live(who: str, det, n_sessions: Optional[int], win_len: int, hop: int, batch: int, ring_len, sample_rates, in_ring_len):
    """The geometry and the rates of `open_stream` (who = "open_stream", n_sessions None: ONE session, sample_rates and in_ring_len its
    two scalars) or of `open_bank` (who = "open_bank"), checked in full before any device work.  -> (cap, rec_cap, rs, in_len): the
    samples per ring, the rows of the record (one group), and per session (rate, L, M, half) and the samples of its input ring - None
    for a session at 44.1 kHz."""
    bank = n_sessions is not None
    n = n_sessions if bank else 1
    if n < 1 or n > 65535:
        raise ValueError("%s: n_sessions = %d (1 .. 65535)" % (who, n))
    if hop < 1:
        raise ValueError("%s: hop = %d: the windows must advance by at least one sample" % (who, hop))
    if batch < 1 or batch > 1024:
        raise ValueError("%s: batch = %d (1 .. 1024)" % (who, batch))
    det.front.n_frames(win_len)               # raises on a window too short for the reflect padding
    span = live_group_span(win_len, hop, batch)
    cap = 2 * span if ring_len is None else int(ring_len)
    if cap < span:
        raise ValueError("%s: ring_len = %d is shorter than one group of %d windows (%d samples)" % (who, cap, batch, span))

    def record():
        rec_cap = batch * (det.cand_cap if det.cand_cap > 0 else det.STREAM_ROWS_PER_WINDOW)
        if rec_cap > 0x7fffffff // _GroupChain.COLS["bank" if bank else "live"]:
            raise ValueError("%s: a record of %d rows" % (who, rec_cap))
        return rec_cap
    if bank:
        rec_cap = record()                    # a bank sizes its record in front of its rates, a session behind them: which error wins stays
    rates = list(sample_rates) if bank and sample_rates is not None else [sample_rates] * n
    if len(rates) != n:
        raise ValueError("%s: sample_rates has %d entries for %d sessions" % (who, len(rates), n))
    listed = bank and isinstance(in_ring_len, (list, tuple))
    in_lens = list(in_ring_len) if listed else [in_ring_len] * n
    if len(in_lens) != n:
        raise ValueError("%s: in_ring_len has %d entries for %d sessions" % (who, len(in_lens), n))
    rs, in_len = [None] * n, [None] * n
    for s, rate in enumerate(rates):
        if rate is None or int(rate) == 44100:
            continue
        L, M, half = resample_ratio(int(rate))
        least = live_in_ring_min(L, M, half)
        in_cap = 2 * half + M - ((-cap * M) // L) if in_lens[s] is None else int(in_lens[s])      # taps + M + ceil(cap * M / L)
        if in_cap < least:
            raise ValueError("%s: in_ring_len = %d%s is shorter than the %d samples resampling %d Hz needs (%d taps + M = %d + 1, and no "
                             "fewer than a block stages)" % (who, in_cap, " of session %d" % s if bank else "", least, int(rate), 2 * half, M))
        rs[s], in_len[s] = (int(rate), L, M, half), in_cap
    if any(k is not None and rs[s] is None for s, k in enumerate(in_lens)) and (listed or not any(rs)):
        raise ValueError(who + (": in_ring_len goes with sessions at a sample rate other than 44100 (nothing else is resampled)" if bank else
                                ": in_ring_len goes with a sample_rate other than 44100 (nothing is resampled)"))
    return cap, rec_cap if bank else record(), rs, in_len


class _LiveHost:
    """The host side of a `LiveSession` and of a `LiveBank`, which is ONE path: a session is the bank's schedule for one session
    (`audio.live_schedule`), on a chain of its own kind.  Here: the forms a chunk may arrive in and the two pinned staging buffers
    host chunks go through in turn (before a buffer is written again, the wait for the event behind the copy that last read it - two
    pushes back); the rings and, per session at another rate, the input ring and its resampling; the schedule's state
    (`audio.bank_state`); the step loop - ring writes, and per tick one control row out of a pinned table, one replay and one drain of
    the record.

    A subclass names its chain (`kind`: "live" / "bank", `_GroupChain`'s), the int32 columns its results carry in front of the track
    ids (`index_cols`), and turns ticks into control rows of that chain (`_control_table`)."""
    kind, index_cols = None, 0

    def _open(self, who: str, det: AudioDetector, n_sessions: Optional[int], win_len: int, hop: int, batch: int,
              track: Optional[TrackConfig], ring_len, sample_rates, in_ring_len):
        cap, rec_cap, rs, in_len = _plan_live(who, det, n_sessions, win_len, hop, batch, ring_len, sample_rates, in_ring_len)
        n, C, dev = len(rs), det.net.spec.in_channels, det.device
        self.det, self.C, self.track, self.n_sessions = det, C, track, n
        self.win_len, self.hop, self.batch, self.ring_len = win_len, hop, batch, cap
        self.state, self.ended, self.closed = bank_state(n), [False] * n, False       # per session: flushed, no pushes until its reset
        self._rs, self._in_len, self._in_rings, self._in_written = rs, in_len, [None] * n, [0] * n
        self._stage = [None, None]                # pinned uint8 staging buffers of host chunks, used in turn
        self._stage_ev = [torch.cuda.Event(), torch.cuda.Event()]
        self._pushes = 0
        self.launches = {"staging_copies": 0}     # H2D copies of host chunks through the staging buffers
        for s, r in enumerate(rs):
            if r is not None:
                if det.resampler is None:
                    det.resampler = Resampler(dev)
                det.resampler._bank(r[0], 44100)          # the filter bank goes to the device now, not in the first push
                self._in_rings[s] = torch.zeros(C, in_len[s], device=dev)
        # the record's host copy goes in front of the chain's buffers: allocated behind them, a push that completes a group at batch = 1
        # took some 15 us longer in the median (profiles/live_host_path_notes.md)
        self._h_blob = torch.zeros(_GroupChain.COLS[self.kind] * rec_cap + 2, dtype=torch.int32, pin_memory=True)
        self._h_flags = torch.zeros(1 + 2 * n, dtype=torch.int32, pin_memory=True)       # detector overflow; per session {next_id, overflow}
        source = torch.zeros((n, C, cap) if self.kind == "bank" else (C, cap), device=dev)
        self._rings = list(source.unbind(0)) if self.kind == "bank" else [source]        # session s's ring
        self.chain = chain = _GroupChain(det, self.kind, source, True, win_len, batch, rec_cap, track)
        self._h_ctl = torch.zeros(1, chain.cur.numel(), dtype=torch.int64, pin_memory=True)
        chain.prepare()                           # the warm-up group reads the zeroed rings: window 0 (of session 0), nothing recorded

    def _stage_buffer(self, nbytes: int) -> torch.Tensor:
        """the pinned staging buffer whose turn it is, at least nbytes long, free to be written; `_staged` follows its upload"""
        k = self._pushes & 1
        self._stage_ev[k].synchronize()           # the copy that last read this buffer (two pushes back) is done
        if self._stage[k] is None or self._stage[k].numel() < nbytes:
            self._stage[k] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        return self._stage[k]

    def _staged(self):
        """behind the copy out of `_stage_buffer`'s buffer: the event its next writer waits for, and the turn passes on"""
        self._stage_ev[self._pushes & 1].record()
        self._pushes += 1
        self.launches["staging_copies"] += 1

    def _to_device(self, host: torch.Tensor) -> torch.Tensor:
        """a host tensor -> a contiguous device copy through the pinned staging buffer whose turn it is"""
        nbytes = host.numel() * host.element_size()
        pinned = self._stage_buffer(nbytes)[:nbytes].view(host.dtype).view(host.shape)
        pinned.copy_(host)
        dev = pinned.to(self.det.device, non_blocking=True)
        self._staged()
        return dev

    def _float_checked(self, chunk) -> torch.Tensor:
        """push's argument, checked -> a float32 [C, n] tensor, where it is (host or device)"""
        if isinstance(chunk, np.ndarray):
            if chunk.dtype != np.float32:
                raise ValueError("push takes float32 [%d, n] samples, found %s" % (self.C, chunk.dtype))
            chunk = torch.from_numpy(chunk if chunk.flags.writeable else chunk.copy())
        if not isinstance(chunk, torch.Tensor) or chunk.dim() != 2 or chunk.dtype != torch.float32 or chunk.shape[0] != self.C or \
                chunk.shape[1] < 1:
            raise ValueError("push takes float32 [%d, n] samples, n >= 1" % self.C)
        return chunk

    def _float_chunk(self, chunk) -> torch.Tensor:
        """push's argument -> float32 [C, n] on the device, rows at least n apart, unit stride along the samples"""
        chunk = self._float_checked(chunk)
        if not chunk.is_cuda:
            chunk = self._to_device(chunk)
        elif chunk.stride(1) != 1 or chunk.stride(0) < chunk.shape[1]:
            chunk = chunk.contiguous()
        return chunk

    def _pcm_checked(self, raw, width: int):
        """push_pcm's arguments, checked -> (uint8 frames where they are - a host or device tensor - bytes per frame)"""
        width = int(width)
        if width not in (2, 3, 4):
            raise ValueError("push_pcm: width = %d (2, 3 or 4 bytes per sample)" % width)
        if isinstance(raw, (bytes, bytearray, memoryview)):
            raw = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy())
        if not isinstance(raw, torch.Tensor) or raw.dtype != torch.uint8 or raw.dim() != 1:
            raise ValueError("push_pcm takes bytes, a bytearray or a one-dimensional uint8 tensor")
        fb = self.C * width
        if raw.numel() < fb or raw.numel() % fb:
            raise ValueError("push_pcm: %d bytes are not whole frames of %d x %d bytes" % (raw.numel(), self.C, width))
        return raw, fb

    def _pcm_chunk(self, raw, width: int):
        """push_pcm's arguments -> (uint8 frames on the device, bytes per frame)"""
        raw, fb = self._pcm_checked(raw, width)
        return (raw.contiguous() if raw.is_cuda else self._to_device(raw)), fb

    # ---- state
    def _reset(self, s: int):
        """a new recording on session s: position, window count and input position back to 0, its queued windows dropped, its tracker
        zeroed; open for pushes again"""
        self.state, self.ended[s], self._in_written[s] = bank_reset(self.state, s), False, 0
        self.chain.zero_tracks(s)

    def close(self):
        """Releases the buffers and the graph."""
        if not self.closed:
            torch.cuda.synchronize()
            self.closed = True
            self.chain = self._h_blob = self._stage = self._rings = None
            self._in_rings = [None] * self.n_sessions
            if self.det._held is self:
                self.det._held = None

    # ---- ticks
    def _drain(self):
        """Waits for the device once, behind one copy of the record and the overflow flags; -> the record's arrays, the record emptied"""
        det, chain = self.det, self.chain
        self._h_blob.copy_(chain.blob, non_blocking=True)
        self._h_flags[0:1].copy_(det.overflow, non_blocking=True)
        if self.track is not None:
            self._h_flags[1:].copy_(chain.trk_state[1].view(-1), non_blocking=True)
        chain.rec_state.zero_()
        torch.cuda.synchronize()
        det.last_cls, det.last_reg = chain.cls, chain.reg
        h = self._h_blob.numpy()
        return chain.read(lambda lo, hi: h[lo:hi].copy(), int(self._h_flags[0]), int(self._h_flags[2::2].max()) if self.track is not None else 0)

    def concat(self, parts: list):
        """what several calls returned -> one result of the same form; no parts: the empty one"""
        if not parts:
            return (np.zeros((0, 6), np.float32),) + tuple(np.zeros(0, np.int32) for _ in range(self.index_cols + (self.track is not None)))
        return tuple(parts[0]) if len(parts) == 1 else tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))

    def _control_table(self, runs: list, out: np.ndarray):
        """runs: [(session, window), ...] per tick -> the control rows of this chain's kind, written into out"""
        raise NotImplementedError

    @torch.no_grad()
    def _run(self, steps: list, write=None):
        """the steps of `bank_schedule` / `bank_step`; write(offset into the chunk, samples, session, absolute position) queues one ring
        write.  The control rows of a call's ticks lie in one pinned table that is only rewritten after that call's final wait."""
        runs = [st[1] for st in steps if st[0] == "run"]
        if self._h_ctl.shape[0] < len(runs):
            self._h_ctl = torch.zeros(len(runs), self._h_ctl.shape[1], dtype=torch.int64, pin_memory=True)
        table = self._h_ctl
        if runs:                                  # most pushes complete no tick: nothing to lay out
            self._control_table(runs, table.numpy())
        parts, k = [], 0
        for st in steps:
            if st[0] == "write":
                write(st[2], st[3] - st[2], st[1], st[2])
            else:
                if k:
                    parts.append(self._drain())   # the record holds one tick
                self.chain.run(table[k])
                if self.kind == "bank":
                    self.ticks.append(list(st[1]))       # a session's ticks are its groups: it keeps no list
                k += 1
        if k:
            parts.append(self._drain())
        return self.concat(parts)

    def _produce(self, s: int, final: bool):
        """session s at another rate: the 44.1 kHz samples its input so far allows (final: up to the recording's end), through the
        schedule: every ring write is one `mmd_ring_resample` from its input ring"""
        rate, L, M, half = self._rs[s]
        ready = live_resample_ready(self._in_written[s], L, M, half, final)
        steps, state = bank_schedule(self.state, s, ready - self.state[0][s], self.win_len, self.hop, self.batch, self.ring_len)
        rs, in_ring, ring, n_valid = self.det.resampler, self._in_rings[s], self._rings[s], self._in_written[s]
        out = self._run(steps, lambda lo, cnt, _, pos: rs.ring_resample_into(in_ring, n_valid, rate, ring, pos, pos + cnt))
        self.state = state
        return out

    def _advance(self, s: int, n: int, write):
        """one chunk of n samples for session s; write(offset into the chunk, samples, ring, its length, absolute position)"""
        if self._rs[s] is not None:
            _, L, M, half = self._rs[s]
            parts, off = [], 0
            for cnt, _ in live_pieces(n, self._in_written[s], self.state[0][s], L, M, half, self._in_len[s]):
                write(off, cnt, self._in_rings[s], self._in_len[s], self._in_written[s])
                self._in_written[s] += cnt
                off += cnt
                parts.append(self._produce(s, False))
            return self.concat(parts)
        base, ring, cap = self.state[0][s], self._rings[s], self.ring_len
        steps, state = bank_schedule(self.state, s, n, self.win_len, self.hop, self.batch, self.ring_len)
        out = self._run(steps, lambda lo, cnt, _, pos: write(lo - base, cnt, ring, cap, pos))
        self.state = state
        return out

    def _step(self):
        """the windows that are ready but wait for a full tick, now: one short tick (nothing with none waiting)"""
        steps, self.state = bank_step(self.state)
        return self._run(steps)

    # ---- chunks
    def _push(self, s: int, chunk):
        self._check_open(pushing=True, session=s)
        chunk = self._float_chunk(chunk)
        ptr, stride = chunk.data_ptr(), chunk.stride(0)
        return self._advance(int(s), chunk.shape[1], lambda off, cnt, ring, cap, pos: _lib.call("mmd_ring_push", ptr + 4 * off, stride, self.C,
                                                                                                cnt, ring, cap, pos))

    def _push_pcm(self, s: int, raw, width: int):
        self._check_open(pushing=True, session=s)
        raw, fb = self._pcm_chunk(raw, width)
        width, ptr = int(width), raw.data_ptr()
        return self._advance(int(s), raw.numel() // fb, lambda off, cnt, ring, cap, pos: _lib.call("mmd_ring_push_pcm", ptr + fb * off, cnt,
                                                                                                   self.C, width, ring, cap, pos))

    @torch.no_grad()
    def flush(self):
        """Ends the recording - a bank: all of them.  A session at another rate first produces its recording's last outputs (ascending
        sessions; the full ticks they complete run); then the short last tick runs - the complete windows no full tick took, padded by
        repeating the last one - and its results are returned; a tail shorter than a window is dropped, as `detect_stream` drops it.
        Afterwards a session takes pushes again only behind its `reset`."""
        self._check_open()
        parts = [self._produce(s, True) for s in range(self.n_sessions) if self._rs[s] is not None and not self.ended[s]]
        self.ended = [True] * self.n_sessions
        return self.concat(parts + [self._step()]) if parts else self._step()


class LiveSession(_LiveHost):
    """A recording that arrives in chunks (`AudioDetector.open_stream`).  `push` / `push_pcm` write a chunk into a ring of samples on the
    device and return the results of the windows the chunk COMPLETED - (rows float32 [R, 6], window int32 [R]), with tracking also
    track int32 [R], in the dtypes and order of `detect_stream` / `track_stream`; window indices count from the start of the recording
    - or empty arrays; `flush` ends the recording; `reset` starts the next one; `close` releases the buffers.

    Grouping does not depend on chunking.  Windows run in groups of exactly `batch` consecutive windows, in window order; a group
    runs as soon as its last sample has been pushed; only `flush` runs a shorter group (padded by repeating its last window, the
    padding not recorded) and drops a tail shorter than a window.  These are the groups `detect_stream` forms over the whole
    recording, and equal groups give equal bits: for ANY way of cutting a recording into chunks, what the pushes and `flush` return,
    concatenated, is bit for bit what `detect_stream` / `track_stream` return for the whole recording at the same win_len, hop, batch,
    tracker settings and detector.  (Nothing more is promised: another batch gives other groups.)  Results therefore come up to
    `batch` windows late: batch = 1 is the low-latency setting.

    The ring (`audio.live_schedule`) holds absolute sample p at slot p % ring_len.  A push alternates ring writes and group runs, and
    a write never passes the first sample of the next group to run plus ring_len, so no sample a pending window needs is overwritten
    whatever the chunk's length - also one longer than the ring.  With hop > win_len the samples between groups are skipped.  On the
    host this is a `LiveBank`'s path for one session (`_LiveHost`): the groups are the ticks of `audio.bank_schedule`, the short last
    group is `audio.bank_step`'s tick; only the chain - its kernels, its control row, its 8-word record - is the session's own.

    One graph of the chain ring front end -> resize -> forward -> decode -> NMS [-> track update] -> record append is captured when
    the session opens (`AudioDetector.live_captures`; with use_graph = False the chain runs eagerly); the ring, the control row and the record keep their addresses, so it serves
    every group of every recording of the session.  The record holds the rows of ONE group (batch x cand_cap, or batch x
    STREAM_ROWS_PER_WINDOW with cand_cap = 0); a group with more raises the RuntimeError of `detect_stream`.

    Synchronisation: a push that completes no group only queues its ring write and returns.  A push that completes a group waits for
    the device once, at its end, behind ONE copy of the record (rows, windows, track ids and count are one block of memory) and the
    two overflow flags into pinned host memory.  A push that completes several groups empties the record that way before each further
    group.  Host chunks go through two pinned staging buffers used in turn; before a buffer is written again the session waits for
    the event behind the copy that last read it - two pushes back - never for the detection chain.  The control rows of a push's
    groups lie in one pinned table that is only rewritten after that push's final wait.

    Another sample rate (`open_stream(sample_rate=R)`, L / M = 44100 / R in lowest terms, a filter of taps = 2 * half taps).  `push` /
    `push_pcm` then take samples at R.  The session owns a second ring, in_ring [8, in_ring_len] of input-rate samples; the chunk is
    written there by the same two writers (in pieces of at most in_ring_len - taps - M samples), and after each piece the outputs
    whose last tap has arrived (`audio.live_resample_ready`) are handed to `audio.live_schedule` exactly as a 44.1 kHz push of that
    many samples: every ring write of the schedule becomes one `mmd_ring_resample` for just those outputs - what the schedule skips
    (hop > win_len) is never computed - and the group runs are untouched.  The captured graph is the same; the resampling launches sit
    outside it, like the ring writes, and the synchronisation rules above hold as they stand.  `flush` first produces the outputs up to
    `audio.resample_len` of the total pushed, the filter's tail reading zeros as it does at the end of a whole recording, runs the
    groups that completes, then the short last group.  The contract: for ANY way of cutting a recording at rate R into chunks, what
    the pushes and `flush` return, concatenated, is bit for bit what `detect_stream` / `track_stream` return for
    `Resampler.resample(whole recording, R)` at the same settings - `mmd_ring_resample` forms the sums of `mmd_resample_poly`, and an
    output depends on its 2 * half inputs alone.  Results come `half` input samples later (1.5 ms at 48 kHz)."""

    kind, index_cols = "live", 1              # the single-source chain; results (rows, window[, track])

    def __init__(self, det: AudioDetector, win_len: int, hop: int, batch: int, track: Optional[TrackConfig], ring_len: Optional[int],
                 sample_rate: Optional[int] = None, in_ring_len: Optional[int] = None):
        self._open("open_stream", det, None, win_len, hop, batch, track, ring_len, sample_rate, in_ring_len)

    # ---- the one session's state, as scalars: samples written, the next group to run, and what a session at another rate keeps
    written = property(lambda self: self.state[0][0])
    group = property(lambda self: self.state[1][0] // self.batch)     # fewer than batch windows wait: next window // batch
    flushed = property(lambda self: self.ended[0])
    rs = property(lambda self: self._rs[0])
    in_ring = property(lambda self: self._in_rings[0])
    in_ring_len = property(lambda self: self._in_len[0])
    in_written = property(lambda self: self._in_written[0])

    def _check_open(self, pushing: bool = False, session: int = 0):
        if self.closed:
            raise RuntimeError("this live session is closed (the detector holds one stream or session at a time)")
        if pushing and self.flushed:
            raise RuntimeError("the recording was flushed: reset() starts the next one")

    def _control_table(self, runs: list, out: np.ndarray):
        """a tick [(0, w0), ...] is the group of those windows: its starts, and its first window"""
        _GroupChain.control_table([([w * self.hop for _, w in tick], tick[0][1]) for tick in runs], self.batch, out)

    def reset(self):
        """Starts a new recording on the same session: position 0 (the input position too), window 0, the tracker zeroed (ids start at
        0 again), the record emptied; the graph, the rings and every buffer stay (they need no clearing: no window reads a slot this
        recording has not written, and the resampler reads zeros for whatever this recording has not pushed)."""
        self._check_open()
        self.chain.rec_state.zero_()
        self._reset(0)

    def push(self, chunk):
        """chunk: float32 [8, n], n >= 1, a device or host tensor or a numpy array: the next n samples of every microphone (at the
        session's sample_rate)"""
        return self._push(0, chunk)

    def push_pcm(self, raw, width: int):
        """raw: bytes, a bytearray or a uint8 tensor (host or device) of whole frames of interleaved little-endian signed PCM, 8 channels
        of `width` = 2, 3 or 4 bytes, as `wave.readframes` returns them; decoded on the device exactly as `Resampler.pcm_to_float`
        decodes (`mmd_ring_push_pcm`).  Otherwise as `push`."""
        return self._push_pcm(0, raw, width)


class LiveBank(_LiveHost):
    """Several recordings that arrive in chunks, side by side (`AudioDetector.open_bank`): n_sessions rings [n_sessions, 8, ring_len]
    and n_sessions trackers behind ONE chain and one captured graph.  `push(s, chunk)` / `push_pcm(s, raw, width)` write a chunk of
    session s into its ring (the argument forms of `LiveSession`; at 44.1 kHz unless the session was opened at another rate, below)
    and return the results of the ticks the chunk completed; `push_all` / `push_all_pcm` take one chunk of several sessions in one call; `step()` runs the pending windows now; `flush()` is `step()` and ends all recordings;
    `reset(s)` starts a new recording on session s; `close()` releases the bank.

    The schedule (`audio.bank_schedule`).  Window w of session s is ready once its last sample w * hop + win_len - 1 has been pushed;
    ready windows enter one FIFO in the order they complete; a TICK - one forward pass - runs exactly when the FIFO holds `batch`
    windows and takes all of them, in FIFO order.  With batch = n_sessions and sources that advance together, a tick is one fresh
    window of every session: no result waits for later windows of its own recording.  `ticks` lists, per tick run so far, its
    [(session, window), ...]; only `step` / `flush` run a shorter tick (1 .. batch-1 windows, padded by repeating the last one, the
    padding not recorded).  A write to session s never passes (first window of s not yet run) * hop + ring_len, so no pending window
    loses a sample whatever the chunk's length.

    Results: every call returns (rows float32 [R, 6], session int32 [R], window int32 [R][, track int32 [R]]), tick by tick, inside a
    tick in its window order, inside a window in `detect`'s order - or empty arrays.  Window indices count within the session's
    recording; track ids count per session from 0.  `concat` joins several results.

    The contract.
    (a) The rows of tick k are bit for bit what `detect` returns for the stack of that tick's windows (`ticks[k]`, a short tick padded
        by repetition) at batch size `batch`.
    (b) With a tracker, the track ids of session s over a whole run equal `tracker.track_rows(rows_s, window_s, n_windows_s, cfg,
        device)` on that session's own returned rows: every session has its own tracker state (`mmd_track_update_bank`), which sees
        that session's windows alone, in order.
    (c) The ticks depend only on the order in which windows complete, never on how a session's audio was cut into pushes.
    Nothing is promised about a window's bits across different tick compositions.

    One graph of the chain rings front end -> resize -> forward -> decode -> NMS [-> track update] -> record append is captured when
    the bank opens (`AudioDetector.bank_captures`; with use_graph = False the chain runs eagerly) and serves every tick of every
    recording (`bank_replays`).  The control row - int64 starts[batch] | int32 sess[batch] | int32 win[batch] | int32 {n_valid, pad} - is
    one contiguous block, copied per tick out of a pinned table.  The record holds the rows of ONE tick (batch x cand_cap, or batch x
    STREAM_ROWS_PER_WINDOW with cand_cap = 0); a tick with more raises the RuntimeError of `detect_stream`.

    Synchronisation follows `LiveSession`: a push that completes no tick only queues its ring write; a push that completes ticks
    drains the record once per tick, behind one copy of the block (rows, windows, track ids, sessions, count) and the overflow
    flags into pinned host memory; host chunks go through the two pinned staging buffers under the same event rule.

    Sessions at other rates (`open_bank(sample_rates=...)`; with none the bank has no input ring and no resampler, and nothing of
    this runs).  A session s at rate R_s owns an input ring in_rings[s] [8, in_ring_len[s]] of input-rate samples, and its pushes are
    `LiveSession`'s: the chunk goes into that ring in pieces of at most in_ring_len - taps - M samples; after each piece the
    outputs whose last tap has arrived (`audio.live_resample_ready`) are handed to `audio.bank_schedule` exactly as a 44.1 kHz push of
    that many samples; every "write" step becomes one resampling of that output range into the session's ring - what the schedule
    skips is never computed - and the ticks are untouched.  `reset(s)` also resets the session's input position.  `flush()` first
    produces, for every such session in ascending order, the outputs up to `audio.resample_len` of what it was pushed (the filter's
    tail reads zeros), running the full ticks that completes, then runs the short tick and ends all recordings.
    (d) The 44.1 kHz samples session s's ring receives are bit for bit `Resampler.resample(whole recording of s, R_s)`, and the
        bank's ticks and bytes equal those of a 44.1 kHz bank that is fed those resampled recordings, cut where
        `live_resample_ready` says the outputs become available.

    A round of chunks (`push_all(chunks)` / `push_all_pcm(chunks, width)`: a mapping, or a sequence of pairs, from session to a chunk
    in `push`'s / `push_pcm`'s forms; width: one int, or one per session - a mapping, or a sequence indexed by session).  Result,
    ticks and bytes are EXACTLY those of `push(s, chunk_s)` for the sessions in ascending order.  The host works out that
    sequential schedule first (`audio.bank_round`).  Where every chunk is one input piece, every session gets at most one ring write
    and no write passes (first window of s not run at the start of the call) * hop + ring_len - so that a write moved in front of
    the call's ticks overwrites nothing a pending window needs - the round takes the fast path: all host chunks and the two
    descriptor tables are packed into the staging buffer whose turn it is (payloads aligned to 16 bytes, the same event rule), go
    to the device in ONE copy, ONE `mmd_rings_push` writes the input rings of the sessions at other rates and the rings of the
    44.1 kHz sessions, at most ONE `mmd_rings_resample` makes the 44.1 kHz samples of the others, and the ticks run in order with a
    drain per tick.  Any other round - and any round with a device-tensor chunk - is the sequential pushes.  `launches` counts
    "fast_rounds", "fallback_rounds", "rings_push", "rings_resample" (the batched launches) and "staging_copies"."""

    kind, index_cols = "bank", 2              # the chain of several sources; results (rows, session, window[, track])

    def __init__(self, det: AudioDetector, n_sessions: int, win_len: int, hop: int, batch: int, track: Optional[TrackConfig],
                 ring_len: Optional[int], sample_rates: Optional[Sequence] = None, in_ring_len=None):
        self.ticks = []
        self._open("open_bank", det, n_sessions, win_len, hop, batch, track, ring_len, sample_rates, in_ring_len)
        self.launches.update(fast_rounds=0, fallback_rounds=0, rings_push=0, rings_resample=0)

    # ---- per session: (rate, L, M, half), the input ring, its length - None at 44.1 kHz - and the input samples pushed so far
    rs = property(lambda self: self._rs)
    in_rings = property(lambda self: self._in_rings)
    in_ring_len = property(lambda self: self._in_len)
    in_written = property(lambda self: self._in_written)

    def _check_open(self, pushing: bool = False, session: Optional[int] = None):
        if self.closed:
            raise RuntimeError("this live bank is closed (the detector holds one stream, session or bank at a time)")
        if session is not None and not (isinstance(session, (int, np.integer)) and 0 <= session < self.n_sessions):
            raise ValueError("session %r of a bank of %d" % (session, self.n_sessions))
        if pushing and self.ended[session]:
            raise RuntimeError("the recordings were flushed: reset(%d) starts the next one on this session" % session)

    def _control_table(self, runs: list, out: np.ndarray):
        _GroupChain.bank_control_table(runs, self.batch, self.hop, out)

    def reset(self, s: int):
        """Starts a new recording on session s: its position and window count back to 0, its tracker zeroed (ids start at 0 again),
        its queued windows dropped, its input position (a session at another rate) back to 0; the other sessions, the graph, the rings
        and every buffer stay.  After a `flush` it reopens session s alone for pushes."""
        self._check_open(session=s)
        self._reset(int(s))

    def step(self):
        """Runs the windows that are ready but wait for a full tick, now: one short tick (nothing with none waiting)."""
        self._check_open()
        return self._step()

    # ---- chunks
    def push(self, s: int, chunk):
        """chunk: float32 [8, n], n >= 1, a device or host tensor or a numpy array: the next n samples of session s (at 44.1 kHz, or at
        the rate the session was opened with)"""
        return self._push(s, chunk)

    def push_pcm(self, s: int, raw, width: int):
        """raw: whole frames of interleaved little-endian signed PCM of session s, as `LiveSession.push_pcm` takes them"""
        return self._push_pcm(s, raw, width)

    # ---- a round of chunks
    def _round_items(self, chunks) -> list:
        """push_all's mapping or sequence of pairs -> [(session, chunk), ...] in ascending session order, every session open for pushes"""
        items = sorted(chunks.items() if hasattr(chunks, "items") else [tuple(c) for c in chunks], key=lambda c: c[0])
        for k, (s, _) in enumerate(items):
            self._check_open(pushing=True, session=s)
            if k and int(items[k - 1][0]) == int(s):
                raise ValueError("push_all: session %d is named twice" % int(s))
        return [(int(s), c) for s, c in items]

    def push_all(self, chunks):
        """One round: chunks maps sessions to chunks in `push`'s forms (a mapping, or a sequence of (session, chunk) pairs).  Returns
        what `push(s, chunk)` for the sessions in ascending order returns, concatenated - see `LiveBank`."""
        self._check_open()
        return self._round([(s, 0, self._float_checked(c)) for s, c in self._round_items(chunks)])

    def push_all_pcm(self, chunks, width):
        """One round of PCM frames in `push_pcm`'s forms; width: bytes per sample, one int for all sessions, or one per session (a
        mapping, or a sequence indexed by session).  Otherwise as `push_all`."""
        self._check_open()
        if isinstance(width, (int, np.integer)):
            width_of = lambda s: width
        elif hasattr(width, "items"):
            width_of = lambda s: width[s]
        else:
            if len(width) != self.n_sessions:
                raise ValueError("push_all_pcm: %d widths for %d sessions" % (len(width), self.n_sessions))
            width_of = lambda s: width[s]
        return self._round([(s, int(width_of(s)), self._pcm_checked(c, width_of(s))[0]) for s, c in self._round_items(chunks)])

    def _sequential(self, items: list):
        self.launches["fallback_rounds"] += 1
        return self.concat([self.push(s, c) if kind == 0 else self.push_pcm(s, c, kind) for s, kind, c in items])

    @torch.no_grad()
    def _round(self, items: list):
        """items: [(session, kind, checked chunk)], ascending; kind 0: float32 [C, n], else the PCM width of uint8 frames"""
        if not items:
            return self.concat([])
        if any(c.is_cuda for _, _, c in items):
            return self._sequential(items)            # device chunks are where they must be: nothing to pack
        C = self.C
        counts = [c.shape[1] if kind == 0 else c.numel() // (C * kind) for _, kind, c in items]
        pushes = []
        for (s, _, _), n in zip(items, counts):
            if self.rs[s] is None:
                pushes.append((s, [n]))
            else:
                _, L, M, half = self.rs[s]
                pushes.append((s, [out for _, out in live_pieces(n, self.in_written[s], self.state[0][s], L, M, half, self.in_ring_len[s])]))
        fast, steps, state, _ = bank_round(self.state, pushes, self.win_len, self.hop, self.batch, self.ring_len)
        if not fast:
            return self._sequential(items)
        # ---- the fast path.  Layout of the staging buffer: push table | resample table | the chunks, each at a multiple of 16 bytes
        write_of = {st[1]: (st[2], st[3]) for st in steps if st[0] == "write"}
        sends = [(s, kind, c, n) for (s, kind, c), n in zip(items, counts) if self.rs[s] is not None or s in write_of]
        n_rs = sum(1 for s in write_of if self.rs[s] is not None)
        rs_at = len(sends) * RINGS_PUSH_DESC
        at = -(-(rs_at + n_rs * RINGS_RS_DESC) // 16) * 16
        offs = []
        for s, kind, c, n in sends:
            offs.append(at)
            at += -(-(c.numel() * c.element_size()) // 16) * 16
        if sends:
            pinned = self._stage_buffer(at)
            host = pinned.numpy()
            push_tab, rs_tab = host[:rs_at].view(np.int64).reshape(-1, 8), host[rs_at:rs_at + n_rs * RINGS_RS_DESC]
            k_rs = 0
            for k, ((s, kind, c, n), off) in enumerate(zip(sends, offs)):
                nbytes = c.numel() * c.element_size()
                pinned[off:off + nbytes].view(c.dtype).view(c.shape).copy_(c)
                fb = 4 if kind == 0 else C * kind                              # bytes per sample of a row / per frame
                if self.rs[s] is None:                                         # the samples the schedule writes, into the session's ring
                    lo, hi = write_of[s]
                    rings_push_entry(push_tab, k, off + fb * (lo - self.state[0][s]), n, hi - lo, kind, self.chain.source[s], self.ring_len, lo)
                    continue
                rings_push_entry(push_tab, k, off, n, n, kind, self.in_rings[s], self.in_ring_len[s], self.in_written[s])
                if s in write_of:                                              # and the outputs the schedule writes, out of the input ring
                    lo, hi = write_of[s]
                    self.det.resampler.rings_resample_plan(rs_tab, k_rs, self.in_rings[s], self.in_written[s] + n, self.rs[s][0],
                                                           self.chain.source[s], lo, hi)
                    k_rs += 1
            dev = pinned[:at].to(self.det.device, non_blocking=True)
            self._staged()
            rings_push_into(dev, push_tab, dev, len(sends), C)
            self.launches["rings_push"] += 1
            if n_rs:
                self.det.resampler.rings_resample_into(rs_tab, dev[rs_at:], n_rs, C)
                self.launches["rings_resample"] += 1
        for (s, _, _), n in zip(items, counts):
            if self.rs[s] is not None:
                self.in_written[s] += n
        out = self._run([st for st in steps if st[0] == "run"])
        self.state = state
        self.launches["fast_rounds"] += 1
        return out

