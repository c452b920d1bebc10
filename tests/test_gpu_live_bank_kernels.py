"""Live session bank on the GPU, the three kernels: the rings front end (mmd_melspec_windows_rings) against mmd_melspec_windows_ring per
session bit for bit, the per-session tracker (mmd_track_update_bank) against mmd_track_update on each session's windows alone, and the
record append with per-row tables (mmd_det_record_append_bank) against numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, WIN, CAP, NS = 8, 4096, 7001, 3             # 7001: no multiple of the hop (1531), of 4 or of 256
BIG = 1 << 31
_CACHE = {}


def _front():
    from mm_distillnet_amd.audio import MelFrontEnd
    if "front" not in _CACHE:
        _CACHE["front"] = MelFrontEnd(DEV)
    return _CACHE["front"]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- rings front end
GUARD_N = 3 * CAP


def _guarded_rings():
    """three rings of noise in ONE block with a NaN guard of 3 * CAP floats on either side -> (block, rings [3, C, CAP] view)"""
    if "rings" not in _CACHE:
        block = torch.full((2 * GUARD_N + NS * C * CAP,), float("nan"))
        block[GUARD_N:GUARD_N + NS * C * CAP] = torch.randn(NS * C * CAP, generator=torch.Generator().manual_seed(3)) * 0.3
        _CACHE["rings"] = block.to(DEV)
    block = _CACHE["rings"]
    return block, block[GUARD_N:GUARD_N + NS * C * CAP].view(NS, C, CAP)


def _rings_windows(rings, sess, starts, db, out_fill=float("nan"), ws_fill=-1):
    f = _front()
    out = torch.full((len(starts), f.n_mels, f.n_frames(WIN), C), out_fill, device=DEV)
    ws = torch.full((len(starts) * C,), ws_fill, dtype=torch.int32, device=DEV)
    f.melspec_windows_rings_into(rings, torch.tensor(sess, dtype=torch.int32, device=DEV), torch.tensor(starts, dtype=torch.int64, device=DEV),
                                 WIN, db, ws.view(torch.float32), out)
    return out


def _ring_windows(ring, starts, db):
    f = _front()
    out = torch.full((len(starts), f.n_mels, f.n_frames(WIN), C), float("nan"), device=DEV)
    ws = torch.full((len(starts) * C,), -1, dtype=torch.int32, device=DEV)
    f.melspec_windows_ring_into(ring, torch.tensor(starts, dtype=torch.int64, device=DEV), WIN, db, ws.view(torch.float32), out)
    return out


# sessions repeated and out of order; starts: straddling the wrap at an odd offset, no wrap, starting on the last slot, beyond 2^31
SESS = [2, 0, 0, 1]
STARTS = [3 * CAP + 5555, 100, CAP - 1 + 5 * CAP, BIG - BIG % CAP + 6000]


@pytest.mark.parametrize("db", [False, True])
def test_rings_windows_equal_the_ring_entry_point_per_session(db):
    block, rings = _guarded_rings()
    before = block.clone()
    assert [(s % CAP) + WIN > CAP for s in STARTS] == [True, False, True, True] and STARTS[2] % CAP == CAP - 1 and STARTS[3] > BIG       # windows that cross the wrap
    got = _rings_windows(rings, SESS, STARTS, db)
    assert torch.isfinite(got).all()
    for s in range(NS):
        mine = [b for b in range(len(SESS)) if SESS[b] == s]
        want = _ring_windows(rings[s], [STARTS[b] for b in mine], db)
        for k, b in enumerate(mine):
            assert torch.equal(_bits(got[b]), _bits(want[k])), (s, b)
    assert not torch.equal(got[1], got[2]) and not torch.equal(got[0], got[3])
    # a dirty maxima workspace and a dirty output give the same bytes
    again = _rings_windows(rings, SESS, STARTS, db, out_fill=123.5, ws_fill=0x7f7fffff)
    assert torch.equal(_bits(again), _bits(got))
    assert torch.equal(_bits(block), _bits(before))


@pytest.mark.parametrize("db", [False, True])
def test_bad_sessions_and_starts_are_clamped_into_the_rings(db):
    """the guard on either side of the rings is NaN: one sample read from it would show in the output"""
    block, rings = _guarded_rings()
    before = block.clone()
    sess = [-5, NS, 1 << 30, -(1 << 31), 1]
    starts = [CAP - 7, 2 * CAP + 6000, 5, CAP - 1, -100]
    got = _rings_windows(rings, sess, starts, db)
    assert torch.isfinite(got).all()
    want = _rings_windows(rings, [0, NS - 1, NS - 1, 0, 1], starts[:4] + [0], db)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(block), _bits(before))


def test_rings_entry_point_refuses_bad_arguments():
    from mm_distillnet_amd import _lib
    f = _front()
    dll = _lib.LIB.load()
    _, rings = _guarded_rings()
    sess = torch.zeros(2, dtype=torch.int32, device=DEV)
    starts = torch.zeros(2, dtype=torch.int64, device=DEV)
    out = torch.full((2, f.n_mels, f.n_frames(WIN), C), -3.0, device=DEV)
    ws = torch.zeros(2 * C, device=DEV)
    good = dict(rings=rings.data_ptr(), n=NS, ch=C, cap=CAP, sess=sess.data_ptr(), starts=starts.data_ptr(), batch=2, win=WIN,
                bs=f.start.data_ptr(), bl=f.length.data_ptr(), bw=f.band.data_ptr(), stride=f.stride, db=1, ws=ws.data_ptr(),
                out=out.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return dll.mmd_melspec_windows_rings(a["rings"], a["n"], a["ch"], a["cap"], a["sess"], a["starts"], a["batch"], a["win"], a["bs"],
                                             a["bl"], a["bw"], a["stride"], a["db"], a["ws"], a["out"], _lib.stream_ptr())
    bad = [dict(rings=None), dict(sess=None), dict(starts=None), dict(bs=None), dict(bl=None), dict(bw=None), dict(out=None),
           dict(ws=None), dict(n=0), dict(n=-1), dict(ch=0), dict(batch=0), dict(win=512), dict(win=CAP + 1), dict(stride=0),
           dict(stride=1 << 20), dict(db=2), dict(db=-1)]
    for kw in bad:
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert float((out != -3.0).sum()) == 0.0                                      # nothing was launched
    assert call() == 0 and call(db=0, ws=None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ---------------------------------------------------------------------------------------------- per-session tracker
DET_MAX = 256


def _scene(seed, n_windows, big_window=None):
    """seeded boxes with integer corners: moving objects, each missed now and then; window 2 holds two IDENTICAL boxes on top of one
    track (equal IoUs: a tie between detections), window 4 one box that both of two tracks born in window 3 meet with IoU 0.25 (a tie
    between slots), windows 5 and 6 are empty; big_window holds 257 boxes"""
    rng = np.random.default_rng(seed)
    objs = [dict(x=int(rng.integers(0, 90)), y=int(rng.integers(0, 90)), s=int(rng.integers(12, 25)), vx=int(rng.integers(-4, 5)),
                 vy=int(rng.integers(-4, 5)), label=int(rng.choice([6, 14]))) for _ in range(7)]
    windows = []
    for w in range(n_windows):
        dets = []
        for o in objs:
            if rng.random() < 0.85:
                dets.append((o["x"], o["y"], o["x"] + o["s"], o["y"] + o["s"], float(rng.integers(30, 100)) / 100, o["label"]))
            o["x"] += o["vx"]
            o["y"] += o["vy"]
        rng.shuffle(dets)
        if w == 2 and dets:
            dets = dets + [dets[0]]
        if w == 3:
            dets = [(200, 200, 220, 220, 0.9, 6), (230, 200, 250, 220, 0.9, 6)] + dets
        if w == 4:
            dets = [(210, 200, 240, 220, 0.9, 6)] + dets                          # IoU 200 / 800 with both of them
        if w in (5, 6):
            dets = []
        if w == big_window:
            dets = [(3 * (k % 20), 3 * (k // 20), 3 * (k % 20) + 2, 3 * (k // 20) + 2, 0.5, 6) for k in range(DET_MAX + 1)]
        windows.append([tuple(float(v) for v in d) for d in dets])
    return windows


def _pack(windows_of_rows, B, cap_img):
    """rows of up to B windows -> packed [B, cap_img, 6] with junk behind the counts and in the padding windows, cnt [B]"""
    packed = np.full((B, cap_img, 6), 7.5, np.float32)
    cnt = np.full(B, 1 << 30, np.int32)                                           # padding windows: a huge count nobody may follow
    for i, rows in enumerate(windows_of_rows):
        packed[i, :len(rows)] = np.asarray(rows, np.float32).reshape(-1, 6)
        cnt[i] = len(rows) if rows else -3                                        # an empty window: a negative count is clamped
    return torch.from_numpy(packed).to(DEV), torch.from_numpy(cnt).to(DEV)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def test_bank_tracker_equals_the_single_tracker_on_each_session_alone():
    from mm_distillnet_amd import _lib
    from mm_distillnet_amd.tracker import TrackConfig, new_bank_state, new_state
    cfg = TrackConfig(max_tracks=24, iou_min=0.2)
    scenes = [_scene(21, 9), _scene(22, 8, big_window=7), _scene(23, 6)]
    B, cap_img = 4, DET_MAX + 1
    # the groups: (session, window) per row, each session's windows in rising order
    groups = [[(0, 0), (1, 0), (2, 0), (0, 1)],          # session 0 twice
              [(1, 1), (1, 2), (0, 2), (1, 3)],          # session 2 absent, session 1 three times
              [(2, 1), (2, 2), (2, 3), (2, 4)],          # one session alone
              [(0, 3), (1, 4), (0, 4), (1, 5)],
              [(0, 5), (0, 6), (1, 6), (2, 5)],          # the empty windows of sessions 0 and 1
              [(1, 7), (0, 7), (0, 8)]]                  # the 257-box window; n_valid = 3 < B
    assert sorted(q for g in groups for q in g) == sorted((s, w) for s in range(NS) for w in range(len(scenes[s])))
    # reference: every session's windows alone, one window per mmd_track_update call
    want_ids, want_state = {}, []
    for s in range(NS):
        st = new_state(DEV, cfg)
        for w, rows in enumerate(scenes[s]):
            packed, cnt = _pack([rows], 1, cap_img)
            ids = torch.full((cap_img + 2,), -77, dtype=torch.int32, device=DEV)
            _lib.call("mmd_track_update", packed, cnt, 1, cap_img, _i32([1, w]), _i32([0]), cap_img, ids, st[0], st[1], cfg.max_tracks,
                      cfg.iou_min, cfg.beta, cfg.max_age, cfg.birth_score)
            want_ids[s, w] = ids.cpu().numpy()[:len(rows)]
        want_state.append((st[0].cpu().numpy(), st[1].cpu().numpy()))
    assert want_state[1][1][1] == 1 and want_state[0][1][1] == 0 and want_state[2][1][1] == 0      # only the 257-box session overflows
    assert all(int(want_state[s][1][0]) >= 7 for s in range(NS))
    assert (want_ids[0, 2] >= 0).sum() >= 2 and (want_ids[1, 7][DET_MAX:] == -1).all()

    state = new_bank_state(DEV, cfg, NS)
    for g in groups:
        rows_of = [scenes[s][w] for s, w in g]
        packed, cnt = _pack(rows_of, B, cap_img)
        sess = [s for s, _ in g] + [1] * (B - len(g))                             # padding rows name a session: n_valid keeps them out
        win = [w for _, w in g] + [99] * (B - len(g))
        first_count = 5
        total = first_count + sum(len(r) for r in rows_of)
        ids = torch.full((total + 2,), -77, dtype=torch.int32, device=DEV)
        absent = [s for s in range(NS) if s not in sess[:len(g)]]
        before = [(state[0][s].clone(), state[1][s].clone()) for s in absent]
        _lib.call("mmd_track_update_bank", packed, cnt, B, cap_img, _i32([len(g)]), _i32(sess), _i32(win), NS, _i32([first_count]), total,
                  ids, state[0], state[1], cfg.max_tracks, cfg.iou_min, cfg.beta, cfg.max_age, cfg.birth_score)
        got = ids.cpu().numpy()
        assert (got[:first_count] == -77).all() and (got[total:] == -77).all()
        at = first_count
        for (s, w), rows in zip(g, rows_of):
            np.testing.assert_array_equal(got[at:at + len(rows)], want_ids[s, w], err_msg=str((s, w)))
            at += len(rows)
        for s, (slots, glob) in zip(absent, before):                              # an absent session: no word changes, nothing ages
            assert torch.equal(state[0][s], slots) and torch.equal(state[1][s], glob)
    for s in range(NS):
        np.testing.assert_array_equal(state[0][s].cpu().numpy(), want_state[s][0])
        np.testing.assert_array_equal(state[1][s].cpu().numpy(), want_state[s][1])
    assert len({want_state[s][0].tobytes() for s in range(NS)}) == NS              # three different trackers
    with pytest.raises(RuntimeError, match="-22"):
        _lib.call("mmd_track_update_bank", packed, cnt, B, cap_img, _i32([1]), _i32(sess), _i32(win), 0, _i32([0]), total, ids, state[0],
                  state[1], cfg.max_tracks, cfg.iou_min, cfg.beta, cfg.max_age, cfg.birth_score)


# ---------------------------------------------------------------------------------------------- record append
def test_bank_append_against_numpy():
    from mm_distillnet_amd import _lib
    rng = np.random.default_rng(9)
    B, cap_img, rec_cap = 5, 7, 30
    rec_rows = torch.full((rec_cap + 2, 6), -9.0, device=DEV)
    rec_win = torch.full((rec_cap + 2,), -9, dtype=torch.int32, device=DEV)
    rec_sess = torch.full((rec_cap + 2,), -9, dtype=torch.int32, device=DEV)
    rec_state = torch.zeros(2, dtype=torch.int32, device=DEV)
    want_rows, want_win, want_sess = np.full((rec_cap + 2, 6), -9.0, np.float32), np.full(rec_cap + 2, -9, np.int32), np.full(rec_cap + 2, -9, np.int32)
    count = 0
    calls = [(5, [3, 0, 7, 1 << 30, 2]), (3, [4, -6, 5, 7, 7]), (5, [7, 7, 0, 1, 2]), (0, [1, 1, 1, 1, 1])]      # (n_valid, cnt)
    overflowed = []
    for n_valid, cnt in calls:
        rows = rng.standard_normal((B, cap_img, 6)).astype(np.float32)
        sess, win = rng.integers(0, 4, B).astype(np.int32), rng.integers(0, 1 << 20, B).astype(np.int32)
        _lib.call("mmd_det_record_append_bank", torch.from_numpy(rows).to(DEV), _i32(cnt), B, cap_img, _i32([n_valid]),
                  torch.from_numpy(sess).to(DEV), torch.from_numpy(win).to(DEV), rec_rows, rec_win, rec_sess, rec_cap, rec_state[0:1],
                  rec_state[1:2])
        for i in range(n_valid):
            n = max(0, min(cnt[i], cap_img))
            for j in range(n):
                if count + j < rec_cap:
                    want_rows[count + j], want_win[count + j], want_sess[count + j] = rows[i, j], win[i], sess[i]
            count += n
        overflowed.append(count > rec_cap)
        assert rec_state.cpu().tolist() == [count, int(any(overflowed))]
    assert overflowed == [False, False, True, True] and count == 19 + 9 + 17      # the third call overflows; the count stays the true total
    np.testing.assert_array_equal(rec_rows.cpu().numpy().view(np.int32), want_rows.view(np.int32))
    np.testing.assert_array_equal(rec_win.cpu().numpy(), want_win)
    np.testing.assert_array_equal(rec_sess.cpu().numpy(), want_sess)
    assert (want_win[rec_cap:] == -9).all() and (want_sess[:rec_cap] >= 0).all()
    with pytest.raises(RuntimeError, match="-22"):
        _lib.call("mmd_det_record_append_bank", rec_rows, rec_win, 0, cap_img, rec_win, rec_win, rec_win, rec_rows, rec_win, rec_sess, rec_cap,
                  rec_state[0:1], rec_state[1:2])
