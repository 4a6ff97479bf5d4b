"""pointnav-vo_amd — MI355X-native drop-in for PointNav-VO's visual-odometry hot path.

Sub-modules:
  model_spec   architecture/state_dict description (no torch)
  synth        deterministic synthetic weights / inputs (numpy only)
  _lib         ctypes binding of csrc/libpnvo.so (the C ABI of include/pnvo.h); fails loudly if missing
  registry     mirror of the reference's baseline_registry VO-model API
  vo_cnn       nn.Module mirrors registered under the reference's model names (HIP forward)
  trainer      mirror of BaseRLTrainerWithVO (_setup_vo_model / _compute_local_delta_states_from_vo)
  train        VOTrainStep / GeoInvarianceTrainStep: the VO engine's training iteration
  evaluate     GeoInvarianceEvalStep: the VO engine's evaluation pass, metrics accumulated on the device
  policy       PointNavResNetPolicy (resnet_rnn_policy) on the HIP path
  baseline_policy  PointNavBaselinePolicy (SimpleCNN + GRU, the plain PPOTrainer's policy) on the HIP path
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the policy classes by name, loaded on first use (importing them loads torch and libpnvo.so)
    if name in ("PointNavBaselinePolicy", "PointNavResNetPolicy"):
        import importlib
        mod = importlib.import_module("pointnav_vo_amd." + ("baseline_policy" if name == "PointNavBaselinePolicy" else "policy"))
        return getattr(mod, name)
    raise AttributeError(f"module 'pointnav_vo_amd' has no attribute {name!r}")
