"""`monoforce.losses` -> monoforce_amd.losses."""
from monoforce_amd.losses import hm_loss, physics_loss, rotation_difference, slerp, total_variation, translation_difference  # noqa: F401

__all__ = ['rotation_difference', 'translation_difference', 'total_variation', 'hm_loss', 'slerp', 'physics_loss']
