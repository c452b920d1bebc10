"""Streaming tracking: links the boxes of consecutive windows into per-vehicle tracks on the device (`mmd_track_update`, csrc/track.hip).

The rule - a greedy IoU tracker with a constant-velocity alpha-beta model, alpha = 1 - is written out in DESIGN.md (streaming tracking)
and in include/mmdistill.h.  `TrackConfig(assign="optimal")` pairs tracks and boxes by the matching of maximum IoU sum instead of greedily
(`mmd_track_update_assign`; DESIGN.md, tracking evaluation, says when to prefer which).  `AudioDetector.track_stream` launches the kernel inside its captured chain, in front of every group's
record append; `track_rows` runs the same kernel over a detection record that already exists (saved detections)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import _lib

SLOT_WORDS = 16             # int32 words per slot of the state (include/mmdistill.h: mmd_track_update)
DET_MAX = 256               # detections of one window that take part
GROUP_MAX = 1024            # windows per launch
ASSIGN = {"greedy": 0, "optimal": 1}      # the `assign` argument of mmd_track_update_assign / mmd_track_update_bank_assign


@dataclass(frozen=True)
class TrackConfig:
    iou_min: float = 0.3        # smallest IoU at which a track and a detection may be paired
    beta: float = 0.5           # velocity gain
    max_age: int = 2            # a track is freed once it has been missed more than this many windows in a row
    birth_score: float = 0.0    # smallest score at which an unmatched detection starts a track
    max_tracks: int = 64        # live-track slots, 1 .. 256
    assign: str = "greedy"      # "greedy": the largest IoU first; "optimal": the matching of maximum IoU sum per window

    def __post_init__(self):
        if not (0.0 < float(self.iou_min) <= 1.0):
            raise ValueError("TrackConfig: iou_min = %r (0 < iou_min <= 1)" % (self.iou_min,))
        if not (0.0 <= float(self.beta) <= 1.0):
            raise ValueError("TrackConfig: beta = %r (0 .. 1)" % (self.beta,))
        if int(self.max_age) != self.max_age or self.max_age < 0:
            raise ValueError("TrackConfig: max_age = %r (an integer >= 0)" % (self.max_age,))
        if not (float(self.birth_score) == float(self.birth_score)):
            raise ValueError("TrackConfig: birth_score is NaN")
        if int(self.max_tracks) != self.max_tracks or not (1 <= self.max_tracks <= 256):
            raise ValueError("TrackConfig: max_tracks = %r (1 .. 256)" % (self.max_tracks,))
        if not isinstance(self.assign, str) or self.assign not in ASSIGN:
            raise ValueError("TrackConfig: assign = %r ('greedy' or 'optimal')" % (self.assign,))

    def key(self) -> tuple:
        key = (float(self.iou_min), float(self.beta), int(self.max_age), float(self.birth_score), int(self.max_tracks))
        return key if self.assign == "greedy" else key + (self.assign,)


def new_state(device, cfg: TrackConfig) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (slots int32 [max_tracks, 16], glob int32 [2] = {next_id, overflow}) on the device, zeroed: a reset tracker"""
    return (torch.zeros(int(cfg.max_tracks), SLOT_WORDS, dtype=torch.int32, device=device),
            torch.zeros(2, dtype=torch.int32, device=device))


def update(rows: torch.Tensor, cnt: torch.Tensor, ctl: torch.Tensor, rec_count: torch.Tensor, rec_cap: int, rec_track: torch.Tensor,
           state, cfg: TrackConfig):
    """One launch of mmd_track_update on the current stream for the group rows [B, cap_img, 6] / cnt [B] / ctl = {n_valid, first_window}
    - in front of the mmd_det_record_append that advances rec_count (cfg.assign = "optimal": of mmd_track_update_assign)."""
    args = (rows, cnt, rows.shape[0], rows.shape[1], ctl, rec_count, int(rec_cap), rec_track, state[0], state[1], int(cfg.max_tracks),
            float(cfg.iou_min), float(cfg.beta), int(cfg.max_age), float(cfg.birth_score))
    if cfg.assign == "greedy":
        _lib.call("mmd_track_update", *args)
    else:
        _lib.call("mmd_track_update_assign", *args, ASSIGN[cfg.assign])


def new_bank_state(device, cfg: TrackConfig, n_sessions: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """`new_state` for a bank of sessions: (slots int32 [n_sessions, max_tracks, 16], glob int32 [n_sessions, 2]), zeroed"""
    return (torch.zeros(int(n_sessions), int(cfg.max_tracks), SLOT_WORDS, dtype=torch.int32, device=device),
            torch.zeros(int(n_sessions), 2, dtype=torch.int32, device=device))


def update_bank(rows: torch.Tensor, cnt: torch.Tensor, n_valid: torch.Tensor, win_sess: torch.Tensor, win_idx: torch.Tensor,
                rec_count: torch.Tensor, rec_cap: int, rec_track: torch.Tensor, state, cfg: TrackConfig):
    """One launch of mmd_track_update_bank on the current stream: `update` for a group whose row i is window win_idx[i] of session
    win_sess[i], on the state of `new_bank_state` - in front of the mmd_det_record_append_bank that advances rec_count."""
    args = (rows, cnt, rows.shape[0], rows.shape[1], n_valid, win_sess, win_idx, state[0].shape[0], rec_count, int(rec_cap), rec_track,
            state[0], state[1], int(cfg.max_tracks), float(cfg.iou_min), float(cfg.beta), int(cfg.max_age), float(cfg.birth_score))
    if cfg.assign == "greedy":
        _lib.call("mmd_track_update_bank", *args)
    else:
        _lib.call("mmd_track_update_bank_assign", *args, ASSIGN[cfg.assign])


def overflow_message(cfg: TrackConfig, window) -> str:
    """what a set overflow flag means for the record whose window column is `window`"""
    window = np.asarray(window).reshape(-1)
    most = int(np.bincount(window[window >= 0]).max()) if len(window) and (window >= 0).any() else 0
    if most > DET_MAX:
        return "tracker capacity exceeded: a window holds %d detections, the first %d take part" % (most, DET_MAX)
    return "tracker capacity exceeded: more than max_tracks = %d live tracks" % int(cfg.max_tracks)


def track_rows(rows, window, n_windows: int, cfg: TrackConfig, device, group: int = 8, state=None) -> np.ndarray:
    """Track ids for a detection record that already exists: rows float32 [R, 6] (x1, y1, x2, y2, score, label), window int [R]
    (non-decreasing, 0 .. n_windows-1: the pair `detect_stream` returns) -> int32 [R], -1 where a row belongs to no track.

    The record is packed into chunks [group, cap, 6] (cap: the largest number of rows in one window) and run through the kernel
    `track_stream` launches, `group` windows per launch; the host waits once, at the end.  state: buffers of `new_state` to go on from and
    to leave the final state in (default: a fresh, reset tracker).  Raises RuntimeError on overflow, naming the capacity exceeded."""
    rows = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 6))
    window = np.asarray(window).reshape(-1).astype(np.int64)
    n_windows, group, R = int(n_windows), int(group), len(rows)
    if len(window) != R:
        raise ValueError("track_rows: %d rows, %d window indices" % (R, len(window)))
    if group < 1 or group > GROUP_MAX:
        raise ValueError("track_rows: group = %d (1 .. %d)" % (group, GROUP_MAX))
    if R and ((np.diff(window) < 0).any() or window[0] < 0 or window[-1] >= n_windows):
        raise ValueError("track_rows: window indices must be non-decreasing and inside 0 .. n_windows-1")
    if n_windows < 1:
        return np.zeros(0, np.int32)
    counts = np.bincount(window, minlength=n_windows).astype(np.int64)
    cap = max(1, int(counts.max()))
    G = (n_windows + group - 1) // group
    first_row = np.concatenate([[0], np.cumsum(counts)])
    packed = np.zeros((G * group, cap, 6), np.float32)
    if R:
        packed[window, np.arange(R) - first_row[window]] = rows
    cnt = np.zeros(G * group, np.int32)
    cnt[:n_windows] = counts
    ctl = np.array([[min(group, n_windows - g * group), g * group] for g in range(G)], np.int32)
    rec_count = first_row[np.minimum(np.arange(G) * group, n_windows)].astype(np.int32)      # the count an append would have left
    packed_d = torch.from_numpy(packed.reshape(G, group, cap, 6)).to(device)
    cnt_d = torch.from_numpy(cnt.reshape(G, group)).to(device)
    ctl_d, rec_count_d = torch.from_numpy(ctl).to(device), torch.from_numpy(rec_count).to(device)
    rec_track = torch.full((max(R, 1),), -1, dtype=torch.int32, device=device)
    if state is None:
        state = new_state(device, cfg)
    for g in range(G):
        update(packed_d[g], cnt_d[g], ctl_d[g], rec_count_d[g:g + 1], max(R, 1), rec_track, state, cfg)
    torch.cuda.synchronize()
    if int(state[1][1].item()):
        raise RuntimeError(overflow_message(cfg, window))
    return rec_track[:R].cpu().numpy()


def tracks_table(window, track) -> np.ndarray:
    """Host summary of a tracked record: window int [R], track int [R] -> int64 [n_tracks, 4] rows (id, first_window, last_window,
    hits) in rising id order; rows without a track (-1) are left out."""
    window, track = np.asarray(window).reshape(-1).astype(np.int64), np.asarray(track).reshape(-1).astype(np.int64)
    if len(window) != len(track):
        raise ValueError("tracks_table: %d window indices, %d track ids" % (len(window), len(track)))
    keep = track >= 0
    ids, inv, hits = np.unique(track[keep], return_inverse=True, return_counts=True)
    first = np.full(len(ids), np.iinfo(np.int64).max, np.int64)
    last = np.full(len(ids), -1, np.int64)
    np.minimum.at(first, inv, window[keep])
    np.maximum.at(last, inv, window[keep])
    return np.stack([ids, first, last, hits], axis=1).astype(np.int64).reshape(-1, 4)
