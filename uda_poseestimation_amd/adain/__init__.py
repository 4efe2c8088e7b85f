"""The reference's adain/ package (AdaIN decoder pre-training, adain/train/train_*.py) on MI355X kernels: `net` (decoder, vgg, Net with
a differentiable forward) and `function` (calc_mean_std, adaptive_instance_normalization).  `_dropin.alias_adain()` registers them
under the reference's top-level names."""
