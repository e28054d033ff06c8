"""mpc4rl_amd — MI355X-native batched MPC-as-policy engine.

Drop-in for the hot path of MPC-Based-Reinforcement-Learning/mpc4rl (``rlmpc.mpc``): the OCP solve
(acados SQP in the reference, rlmpc/mpc/common/mpc.py:27-96,177-202) and the KKT sensitivities
``dV/dp``, ``dQ/dp``, ``du0*/dp`` (rlmpc/mpc/nlp.py:1341-1424) for a whole batch of instances in one
HIP kernel launch.  The arithmetic lives in ``csrc/`` behind the C ABI of ``include/mpcrl.h``;
PyTorch is used for device memory and streams only.  There is no CPU fallback: importing the solver
classes without ``libmpcrl_hip.so`` raises.
"""
from .problems import OcpDescription, cartpole_ocp, chain_mass_ocp, linear_system_ocp  # noqa: F401
from .batch import BoxBounds, CartpoleCost, ChainTrajectoryJacobian, MPCBatch, SolveResult, StateSens, TrajectoryJacobian, cartpole_cost_of, cartpole_theta  # noqa: F401
from .autograd import MPCFunction, MPCLayer, MPCQFunction, MPCTrajectoryFunction, mpc_backward_terms  # noqa: F401
from .envs import BatchedCartPoleSwingUpEnv, BatchedChainMassEnv, BatchedLinearSystemEnv  # noqa: F401
from .qlearning import BatchedQLearning, qlearning_gn_box_step, qlearning_gn_step, qlearning_gn_terms  # noqa: F401
from .qlearning_cartpole import CartpoleEpisodeStats, CartpoleQLearning, qlearning_td_terms  # noqa: F401
from .qlearning_linear import LinearQLearning, linear_collect_terms, linear_env_par, linear_env_step_terms  # noqa: F401
from .qlearning_chain import ChainQLearning, chain_collect_terms, chain_env_step_terms, chain_theta_bounds  # noqa: F401
from .policy_gradient import (CartpolePolicyGradient, ChainPolicyGradient, DevicePolicyGradient, LinearPolicyGradient, cdpg_step,  # noqa: F401
                              cdpg_terms)
from .td3 import BatchedTD3, ContinuousCritic, DeviceReplayBuffer, MPCActor, MPCTD3Policy  # noqa: F401
from .ppo import BatchedPPO, MPCActorCriticPolicy, ppo_collect_terms, ppo_gae, ppo_linear_collect_terms, ppo_surrogate_terms, ppo_value_terms  # noqa: F401
from .ppo import ppo_chain_collect_terms, ppo_surrogate_terms_nu  # noqa: F401
from .config import cartpole_ocp_from_config, read_config, store_iterate, load_iterate  # noqa: F401
from .mpc import MPC, CartpoleMPC, ChainMassMPC, LinearSystemMPC  # noqa: F401

__all__ = ["OcpDescription", "cartpole_ocp", "linear_system_ocp", "chain_mass_ocp", "MPCBatch", "SolveResult", "BoxBounds", "MPC", "CartpoleMPC",
           "LinearSystemMPC", "ChainMassMPC", "CartpoleCost", "cartpole_cost_of", "cartpole_theta", "TrajectoryJacobian"]
