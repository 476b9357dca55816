"""Occupancy network config (model part of snap/configs/train_occupancy.py:21-58).

As in train_localization.py here, the data / schedule entries of the reference config belong to
the Scenic training harness, which is out of scope; the scalar ones a driver needs are kept as
plain values, and the optimiser's parameter freeze is passed to ``trainer.train_step``.
"""
from snap_amd.configs import defaults
from snap_amd.utils.config_dict import ConfigDict


def get_config() -> ConfigDict:
  model = defaults.occupancy_net()
  model.occupancy_mlp.layers = (128, 256, 1)
  return ConfigDict(
      model_name='occupancy_net', model=model, batch_size=1, rng_seed=0,
      # the encoder is frozen (optimizer_configs.freeze_params_reg_exp): pass it as
      # ``trainer.train_step(..., freeze_params_reg_exp=config.freeze_params_reg_exp)``
      freeze_params_reg_exp='streetview_encoder/',
      # float16 under DynamicScale, as the reference: ``trainer.dtype_and_dynamic_scale(config.dtype_str)``
      dtype_str='float16', voxel_size=0.2, num_rays=10_000,
      lr_configs=dict(base_learning_rate=5e-5), num_training_steps=50_000,
  )
