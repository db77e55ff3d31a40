"""Checkpoint files of the reference trainer (audio_exp_nerf.py:498-525,584-592;
TorsoNeRF/train_torso.py:565-573): ``head.tar`` = {'global_step', 'model_state_dict',
'optimizer', 'latent_codes'}, resume from the naturally-sorted last ``*.tar`` of the run
directory, and warm start from AD-NeRF checkpoints (``ft_path``) whose first / skip / view layers
have other input widths and are dropped.  The AD-NeRF baseline (head_baseline.py:439-457,516-520; test_nerf.py:155-172) has
two forms of its own: the run file ``{'global_step', 'model_state_dict', 'optimizer'}`` with upstream's ``module.`` keys, and
AD-NeRF's four state dicts, read in full and strict (``load_adnerf``) and written (``save_adnerf``).
"""
import os
import re

import torch


def natural_key(s: str):
    return [int(t) if t.isdigit() else t.lower() for t in re.split(r"(\d+)", s)]


def latest_checkpoint(run_dir: str, contains: str = ".tar"):
    """natsorted(listdir)[-1] among names containing '.tar' (audio_exp_nerf.py:516-518), or None.  contains: the substring
    looked for instead -- the torso stage takes 'head.tar', then 'torso.tar' (train_torso.py:489-499)."""
    if not os.path.isdir(run_dir):
        return None
    names = sorted((f for f in os.listdir(run_dir) if contains in f), key=natural_key)
    return os.path.join(run_dir, names[-1]) if names else None


def _with_pose_deltas(ckpt: dict, pose_deltas, expr_deltas=None, background=None):
    """The file gains ``pose_deltas`` [n_frames, 6] only for a run that refines its cameras (pose_refine.PoseRefiner), and
    ``expr_deltas`` [n_frames, dim_expr] / ``background`` [H, W, 3] only for one that refines its expressions / learns its
    background (cond_refine.ExprRefiner / Background)."""
    for key, value in (("pose_deltas", pose_deltas), ("expr_deltas", expr_deltas), ("background", background)):
        if value is not None:
            ckpt[key] = value.detach().clone()
    return ckpt


def save_checkpoint(path: str, network, optimizer, latent_codes, global_step: int, pose_deltas=None, expr_deltas=None,
                    background=None):
    """audio_exp_nerf.py:586-591.  pose_deltas / expr_deltas / background (no counterpart upstream): see ``load_pose_deltas``,
    ``load_expr_deltas``, ``load_background``; all None: upstream's keys."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(_with_pose_deltas({"global_step": global_step, "model_state_dict": network.state_dict(),
                                  "optimizer": optimizer.state_dict() if optimizer is not None else None,
                                  "latent_codes": latent_codes.data}, pose_deltas, expr_deltas, background), path)


def load_pose_deltas(path: str, map_location=None):
    """-> the ``pose_deltas`` [n_frames, 6] a run with pose refinement saved.  A file without them raises: resuming such a run
    from a checkpoint of a run without refinement would silently restart the cameras."""
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    if "pose_deltas" not in ckpt:
        raise KeyError(f"{path} holds no pose_deltas: it was written by a run without pose refinement")
    return ckpt["pose_deltas"]


def _load_key(path, key, map_location, written_by):
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    if key not in ckpt:
        raise KeyError(f"{path} holds no {key}: it was written by a run without {written_by}")
    return ckpt[key]


def load_expr_deltas(path: str, map_location=None):
    """-> the ``expr_deltas`` [n_frames, dim_expr] a run with ``refine_expr`` saved.  A file without them raises, as
    ``load_pose_deltas`` does: resuming from it would silently restart the expressions."""
    return _load_key(path, "expr_deltas", map_location, "expression refinement")


def load_background(path: str, map_location=None):
    """-> the ``background`` [H, W, 3] (float32, unclamped) a run with ``learn_background`` saved.  A file without it raises."""
    return _load_key(path, "background", map_location, "a learned background")


def load_checkpoint(path: str, network, optimizer=None, map_location=None, strict=True):
    """-> (global_step, latent_codes).  Keys and strictness as upstream (:520-524); strict=False: how the torso stage takes the
    head stage's weights (train_torso.py:495)."""
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    network.load_state_dict(ckpt["model_state_dict"], strict=strict)
    if optimizer is not None and ckpt.get("optimizer") is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    return ckpt["global_step"], ckpt["latent_codes"]


DATA_PARALLEL_PREFIX = "module."


def save_baseline_checkpoint(path: str, network, optimizer, global_step: int, pose_deltas=None, background=None):
    """The AD-NeRF baseline's run file (head_baseline.py:516-520): {'global_step', 'model_state_dict', 'optimizer'}, no latent
    codes.  Upstream wraps the network in ``nn.DataParallel`` on this path (:448), so its keys carry ``module.``: they are
    written that way, and upstream's trainer and tester load the file as their own."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(_with_pose_deltas({"global_step": global_step,
                                  "model_state_dict": {DATA_PARALLEL_PREFIX + k: v for k, v in network.state_dict().items()},
                                  "optimizer": optimizer.state_dict() if optimizer is not None else None}, pose_deltas,
                                 None, background), path)


def load_baseline_checkpoint(path: str, network, optimizer=None, map_location=None):
    """-> global_step.  Strict, as upstream (head_baseline.py:455-457); the keys may carry upstream's ``module.`` prefix
    (every one of them) or none."""
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    state = ckpt["model_state_dict"]
    if state and all(k.startswith(DATA_PARALLEL_PREFIX) for k in state):
        state = {k[len(DATA_PARALLEL_PREFIX):]: v for k, v in state.items()}
    network.load_state_dict(state, strict=True)
    if optimizer is not None and ckpt.get("optimizer") is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    return ckpt["global_step"]


ADNERF_KEYS = (("network_fn_state_dict", "face_nerf_coarse"), ("network_fine_state_dict", "face_nerf_fine"),
               ("network_audnet_state_dict", "aud_net"), ("network_audattnet_state_dict", "aud_att_net"))


def load_adnerf(path_or_dict, network, map_location=None):
    """An AD-NeRF checkpoint as what it is (head_baseline.py:439-446, test_nerf.py:155-163): the coarse / fine FaceNeRFs and
    the two audio nets, each dict in full and strict -- a file of another model (other input widths, missing or extra keys)
    raises.  ``network``: a ``head_baseline.Network``.  -> the file's ``global_step`` (None where it records none)."""
    ckpt = path_or_dict if isinstance(path_or_dict, dict) else torch.load(path_or_dict, map_location=map_location,
                                                                          weights_only=False)
    missing = [k for k, _ in ADNERF_KEYS if k not in ckpt]
    if missing:
        raise KeyError(f"not an AD-NeRF checkpoint: no {missing} among {sorted(ckpt)}")
    for key, name in ADNERF_KEYS:
        getattr(network, name).load_state_dict(ckpt[key], strict=True)
    return ckpt.get("global_step")


def save_adnerf(path: str, network, global_step: int):
    """``network`` (a ``head_baseline.Network``) in AD-NeRF's four-dict form: a valid ``--ft_path`` for upstream's baseline
    trainer and tester and for AD-NeRF tooling, and what ``load_adnerf`` reads back unchanged."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(dict({key: getattr(network, name).state_dict() for key, name in ADNERF_KEYS}, global_step=global_step), path)


ADNERF_DROP = ("pts_linears.0.weight", "pts_linears.5.weight", "views_linears.0.weight")


def load_adnerf_finetune(path_or_dict, network, map_location=None):
    """Warm start from an AD-NeRF checkpoint (audio_exp_nerf.py:498-514): the coarse / fine
    FaceNeRF weights minus the three layers whose input width differs, and the audio nets,
    all with strict=False."""
    ckpt = path_or_dict if isinstance(path_or_dict, dict) else torch.load(path_or_dict, map_location=map_location,
                                                                          weights_only=False)
    coarse = {k: v for k, v in ckpt["network_fn_state_dict"].items() if k not in ADNERF_DROP}
    fine = {k: v for k, v in ckpt["network_fine_state_dict"].items() if k not in ADNERF_DROP}
    network.face_nerf_coarse.load_state_dict(coarse, strict=False)
    network.face_nerf_fine.load_state_dict(fine, strict=False)
    network.aud_net.load_state_dict(ckpt["network_audnet_state_dict"], strict=False)
    network.aud_att_net.load_state_dict(ckpt["network_audattnet_state_dict"], strict=False)
    return network
