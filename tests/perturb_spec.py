"""NumPy statement of the sensory perturbation (DESIGN "Synthetic env"): a biased env reports object 1 (observation and
achieved-goal entries 3..5) at fl32(true + b) while its state, kept in self.o, evolves on the true coordinates.
step() of the oracle computes the reward and is_success from _obs()['achieved_goal'], so overriding _obs() is the
whole model (a gym robotics env that biases _get_obs)."""
import numpy as np

from oracle.env import SyntheticMultiTaskArm

BIAS_OFF = np.array([0.15, -0.15, 0.0], np.float32)


class BiasedArm(SyntheticMultiTaskArm):
    def __init__(self, *args, bias=False, bias_off=BIAS_OFF, **kwargs):
        super().__init__(*args, **kwargs)
        self.bias = bool(bias)
        self.bias_off = np.asarray(bias_off, np.float32)

    def _obs(self):
        obs = super()._obs()
        if self.bias:
            if self.nb_tasks < 2:
                raise ValueError('the observation bias acts on object 1, an env of %d task(s) has none' % self.nb_tasks)
            for key in ('observation', 'achieved_goal'):
                obs[key][3:6] = (obs[key][3:6] + self.bias_off).astype(np.float32)
        return obs
