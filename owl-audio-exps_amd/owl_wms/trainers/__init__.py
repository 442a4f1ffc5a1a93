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
    if trainer_id == "sforce_vid":
        from .sf_trainer import SelfForceTrainer
        return SelfForceTrainer
    if trainer_id == "causvid":
        from .causvid_trainer import CausVidTrainer
        return CausVidTrainer
    raise NotImplementedError(f"trainer {trainer_id!r}: of the distillation trainers the self-forcing one "
                              "('sforce_vid', trainers/sf_trainer.py over the rollout and the critic / DMD "
                              "losses of trainers/self_forcing.py) and CausVid ('causvid', trainers/"
                              "causvid_trainer.py over trainers/causvid.py, for game_rft and game_rft_audio) are "
                              "built; the ids 'causvid_vid' and 'ode_distill_vid' are not registered "
                              "(SURVEY.md §2.1)")
