"""gsdyn -- host-side callers of the rasterizer path.

Python mirrors of the reference's own callers of ``diff_gaussian_rasterization`` (the reference is
Python here, so is this): camera record construction, parameter activation, the ``get_loss`` step of
``src/tracking/train_utils.py`` and the one-view-per-GPU data-parallel driver that the north star adds.
Nothing in this package computes a render: every render goes through ``GaussianRasterizer``.
"""
from .camera import setup_camera, look_at_w2c, Rt_to_w2c  # noqa: F401
from .scene import synth_scene_params, synth_ring_cameras, synth_targets  # noqa: F401
from .step import params2rendervar, get_loss, get_loss_views, loss_and_grads_views, LossWeights, initialize_optimizer  # noqa: F401
from .plan import (decode_action, rollout_actions, running_cost, mppi_update, sample_action_seq, clip_actions,  # noqa: F401
                   plan_actions, running_cost_grad, rollout_actions_grad, plan_actions_gd)
from .knn import knn_points  # noqa: F401
from .observe import voxel_down_sample, depth_to_cloud, observe_state  # noqa: F401
from .dyn_train import dynamics_loss, train_dynamics_step  # noqa: F401
from .dyn_data import make_dynamics_batch, draw_batch_randomness  # noqa: F401
from .rigid_fit import umeyama_fit  # noqa: F401
from .train import train, train_timestep, initialize_per_timestep, initialize_post_first_timestep, params2cpu, save_params  # noqa: F401
