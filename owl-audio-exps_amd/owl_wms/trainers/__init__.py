"""Trainer registry (reference: owl_wms/trainers/__init__.py:1-37)."""


def get_trainer_cls(trainer_id):
    if trainer_id == "rft":
        from .rft_trainer import RFTTrainer
        return RFTTrainer
    if trainer_id == "audio_rft":
        from .rft_trainer import AudioRFTTrainer
        return AudioRFTTrainer
    if trainer_id == "av":
        from .rft_trainer import AVRFTTrainer
        return AVRFTTrainer
    raise NotImplementedError(f"trainer {trainer_id!r}: the distillation trainer classes are not built (SURVEY.md "
                              "§2.1).  Their core is: trainers/self_forcing.py has the self-forcing rollout "
                              "(RolloutManager, gradients through the KV-cache decode step) and the critic / DMD "
                              "losses; the trainer class around them (teacher checkpoint, VAE decoder, EMA, "
                              "logging) is not")
