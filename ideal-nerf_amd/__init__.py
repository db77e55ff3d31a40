"""idealnerf_amd: MI355X-native per-ray hot path of IDEAL-NeRF.

Import as ``idealnerf_amd`` (the directory is named ``ideal-nerf_amd``; the alias module
at the repository root makes it importable).  Layout mirrors the reference:

    idealnerf_amd.models.face_nerf.FaceNeRF        <- models/face_nerf.py
    idealnerf_amd.models.audio_net.*               <- models/audio_net.py
    idealnerf_amd.helper                           <- NeRFs/HeadNeRF/helper.py (render math)
    idealnerf_amd.audio_exp_nerf.Network           <- NeRFs/HeadNeRF/train/audio_exp_nerf.py
    idealnerf_amd.agg_aud_exp_nerf.Network         <- NeRFs/HeadNeRF/train/agg_aud_exp_nerf.py (FaceNeRFAgg; train_agg.train)
    idealnerf_amd.head_baseline.Network            <- NeRFs/HeadNeRF/train/head_baseline.py (AD-NeRF baseline; train_baseline.train)
    idealnerf_amd.train_torso.Network              <- NeRFs/TorsoNeRF/train_torso.py (composite)
    idealnerf_amd.parallel                         <- row-band tiling + RCCL all-gather; frame shares + ordered assembly
    idealnerf_amd.clip                             <- the eval / test scripts' clip loops (eval_aud_exp_nerf.py, test_torso.py)
    idealnerf_amd.drive                            <- the same scripts whole: loaders, checkpoints, clip (drive_head, drive_torso, drive_baseline)
"""
__version__ = "0.1.0"

from . import _lib, ops  # noqa: F401
from .models.face_nerf import FaceNeRF, invalidate_packed, set_default_precision, set_render_precision  # noqa: F401
from .models.face_nerf_agg import FaceNeRFAgg  # noqa: F401
from .drive import drive_baseline, drive_head, drive_torso  # noqa: F401
