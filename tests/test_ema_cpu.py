"""CPU: the host side of the student's weight averaging - StepConfig's checks, train.py's cfg keys, the --ema refusals of evaluate.py and
detect.py (before the device is touched), the header's declaration of `mmd_ema_update`, and the store's export / import of buffers
other than its own."""
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "mm-distillnet.cfg")


def _tools():
    sys.path.insert(0, ROOT)
    import train, evaluate, detect
    return train, evaluate, detect


@pytest.mark.parametrize("d", [0, 0.0, 0.5, 0.9998])
def test_step_config_accepts(d):
    from mm_distillnet_amd.step import StepConfig
    assert StepConfig(ema_decay=d).ema_decay == d
    assert StepConfig().ema_decay == 0.0 and StepConfig().ema_warmup is True
    assert StepConfig(ema_decay=0.5, ema_warmup=False).ema_warmup is False


@pytest.mark.parametrize("d", [1.0, -0.1, float("nan"), 1.5, float("inf"), "0.5", None, True])
def test_step_config_refuses(d):
    from mm_distillnet_amd.step import StepConfig
    with pytest.raises(ValueError, match="ema_decay"):
        StepConfig(ema_decay=d)


def test_step_config_refuses_a_warmup_that_is_no_bool():
    from mm_distillnet_amd.step import StepConfig
    with pytest.raises(ValueError, match="ema_warmup"):
        StepConfig(ema_decay=0.5, ema_warmup=1)


def test_train_cfg_keys_absent_mean_off():
    train, _, _ = _tools()
    cfg, _ = train.parse_config(["--config_file", CFG])
    sc = train.step_config(cfg)
    assert sc.ema_decay == 0.0 and sc.ema_warmup is True
    assert train.TR.ema_settings(cfg) == {"ema_decay": 0.0, "ema_warmup": True}
    assert train.TR.ema_validate_setting(cfg) is False
    ov = json.dumps({"ema_decay": 0.9998, "ema_warmup": "False", "ema_validate": "True"})
    cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", ov])
    sc = train.step_config(cfg)
    assert sc.ema_decay == 0.9998 and sc.ema_warmup is False and train.TR.ema_validate_setting(cfg) is True
    for bad in (1.0, -0.1, "nan"):
        cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", json.dumps({"ema_decay": bad})])
        with pytest.raises(ValueError, match="ema_decay"):
            train.step_config(cfg)
    cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", json.dumps({"ema_validate": "True"})])
    with pytest.raises(Exception, match="ema_decay"):
        train.TR.ema_validate_setting(cfg)


@pytest.fixture
def no_device(monkeypatch):
    """any touch of torch.cuda the tools could make on their way to the device fails the test"""
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("set_device", "init", "_lazy_init", "synchronize", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, touched)


@pytest.fixture
def plain_checkpoint(tmp_path):
    path = tmp_path / "checkpoint.0.pth.tar"
    torch.save({"epoch": 1, "state_dict": {"w": torch.zeros(1)}, "best_loss": 1.0, "best_epoch": 0}, path)
    return str(path)


MESSAGE = "holds no `state_dict_ema`.*ema_decay"


def test_evaluate_ema_refuses_a_checkpoint_without_average(no_device, plain_checkpoint):
    _, evaluate, _ = _tools()
    with pytest.raises(ValueError, match=MESSAGE):
        evaluate.main(["--config_file", CFG, "--checkpoint", plain_checkpoint, "--ema"])
    with pytest.raises(ValueError, match="--checkpoint"):
        evaluate.main(["--config_file", CFG, "--ema"])


@pytest.mark.parametrize("flags", [[], ["--window_s", "1.0"], ["--resample"], ["--window_s", "1.0", "--chunk_s", "0.5"]])
def test_detect_ema_refuses_a_checkpoint_without_average(no_device, plain_checkpoint, tmp_path, flags):
    _, _, detect = _tools()
    with pytest.raises(ValueError, match=MESSAGE):
        detect.main(["--config_file", CFG, "--checkpoint", plain_checkpoint, "--input", str(tmp_path / "a.wav"),
                     "--output", str(tmp_path / "o.csv"), "--ema"] + flags)


def test_checkpoint_student_state_picks_the_asked_weights():
    from mm_distillnet_amd import trainer as TR
    raw, avg = {"w": torch.zeros(1)}, {"w": torch.ones(1)}
    c = {"state_dict": raw, "state_dict_ema": avg, "ema_updates": 3}
    assert TR.checkpoint_student_state(c, False, "p") is raw and TR.checkpoint_student_state(c, True, "p") is avg
    assert TR.checkpoint_student_state(raw, False, "p") is raw          # a bare state dict (only_parameters_student_best.<rank>)
    with pytest.raises(ValueError, match=MESSAGE):
        TR.checkpoint_student_state(raw, True, "p")


def test_header_declares_ema_update_as_python_calls_it():
    from mm_distillnet_amd import _lib
    sig = _lib.parse_header()["mmd_ema_update"]
    pair = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    assert sig == pair * 3 + [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    # step.py hands over everything but the stream, which _lib.call appends
    import ast
    import inspect
    import textwrap
    from mm_distillnet_amd.step import DistillEngine
    tree = ast.parse(textwrap.dedent(inspect.getsource(DistillEngine.optimizer_body)))
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and n.args and isinstance(n.args[0], ast.Constant)
             and n.args[0].value == "mmd_ema_update"]
    assert len(calls) == 1 and len(calls[0].args) - 1 == len(sig) - 1


def test_store_exports_and_loads_other_buffers():
    from mm_distillnet_amd.arch import make_spec
    from mm_distillnet_amd.store import ParamStore
    ps = ParamStore(make_spec(0, 8), "cpu", with_grads=False)
    g = torch.Generator().manual_seed(3)
    state = {k: (torch.randn(v.shape, generator=g) if v.dtype.is_floating_point else v) for k, v in ps.export_state().items()}
    ps.load_state(state)
    ps.nbt += 7
    own = [t.clone() for t in (ps.flat, ps.rmean, ps.rvar, ps.nbt)]
    flat, rmean, rvar = torch.zeros_like(ps.flat), torch.zeros_like(ps.rmean), torch.zeros_like(ps.rvar)
    other = {k: (v * 2 if v.dtype.is_floating_point else v) for k, v in state.items()}
    ps.load_state(other, flat=flat, rmean=rmean, rvar=rvar)
    for t, o in zip((ps.flat, ps.rmean, ps.rvar, ps.nbt), own):
        assert torch.equal(t, o)                                          # the store's own buffers were left alone
    out = ps.export_state(flat=flat, rmean=rmean, rvar=rvar)
    assert set(out) == set(state)
    for k, v in out.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 7                                            # the live counter
        else:
            assert torch.equal(v, other[k]), k
    plain = ps.export_state()
    for k, v in plain.items():
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(v, state[k]), k
    with pytest.raises(ValueError, match="go together"):
        ps.load_state(other, flat=flat)
