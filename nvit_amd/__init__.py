"""nvit_amd: MI355X-native nViT hot path (HIP kernels behind the reference's Python API)."""
from .config import ViTConfig, named_config, train_flops_per_image  # noqa: F401


def __getattr__(name):
    # model/ops import torch and bind the HIP library lazily
    if name in ("ViT", "Block", "CrossAttentionBlock", "RMSNorm", "resample_pos_embed"):
        from . import model
        return getattr(model, name)
    if name in ("normalize_matrices", "train_step", "GraphedTrainStep"):
        from . import train
        return getattr(train, name)
    if name in ("predict", "validate", "estimate_loss", "GraphedEval"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("AutoAugment", "AugmentedBatch"):
        from . import augment
        return getattr(augment, name)
    if name == "RandAugment":
        from . import randaug
        return randaug.RandAugment
    if name in ("Mixup", "MixedBatch", "MixedTargets"):
        from . import mix
        return getattr(mix, name)
    if name in ("RandomResizedCrop", "CroppedBatch", "RandomErasing", "ErasedBatch", "ResizeCenterCrop", "CenterCroppedBatch"):
        from . import crop
        return getattr(crop, name)
    if name in ("DeviceDataset", "DeviceLoader", "LoaderBatch"):
        from . import data
        return getattr(data, name)
    if name == "ModelEma":
        from . import ema
        return ema.ModelEma
    if name == "DropPath":
        from . import droppath
        return droppath.DropPath
    if name == "PatchDropout":
        from . import patchdrop
        return patchdrop.PatchDropout
    if name in ("LRSchedule", "layer_decay_groups"):
        from . import schedule
        return getattr(schedule, name)
    if name == "FusedAdamW":
        from . import optim
        return optim.FusedAdamW
    raise AttributeError(name)
