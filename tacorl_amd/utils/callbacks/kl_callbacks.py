"""KL annealing (reference utils/callbacks/kl_callbacks.py; config/callbacks/kl_schedule/{constant,linear,sigmoid}.yaml): at
the start of every training epoch the schedule hands the module its KL weight through `set_kl_beta`.  kl_beta is a launch
argument of the KL kernel, so PlayLMPShell.set_kl_beta drops the captured step graphs when the value changes."""
import math

from ...lightning import CallbackBase


class KLSchedule(CallbackBase):
    """Base: beta(epoch) = 0 before start_epoch, max_kl_beta after end_epoch, `_ramp` in between (both ends included)."""

    def __init__(self, start_epoch: int, end_epoch: int, max_kl_beta: float):
        self.start_epoch, self.end_epoch, self.max_kl_beta = start_epoch, end_epoch, max_kl_beta

    def on_train_epoch_start(self, trainer, pl_module) -> None:
        pl_module.set_kl_beta(self._anneal_fn(pl_module.current_epoch))

    def _anneal_fn(self, epoch):
        if epoch < self.start_epoch:
            return 0.0
        if epoch > self.end_epoch:
            return self.max_kl_beta
        return self._ramp(epoch)

    def _ramp(self, epoch):
        raise NotImplementedError


class KLConstantSchedule(KLSchedule):
    """Leaves the module's own kl_beta alone."""

    def __init__(self):
        pass

    def on_train_epoch_start(self, trainer, pl_module) -> None:
        pass

    def _anneal_fn(self, epoch):
        return None


class KLLinearSchedule(KLSchedule):
    def _ramp(self, epoch):
        return self.max_kl_beta * (epoch - self.start_epoch) / (self.end_epoch - self.start_epoch)


class KLSigmoidSchedule(KLSchedule):
    """A logistic curve across the ramp: 12 of its units span [start_epoch, end_epoch], centred on the middle."""

    def _ramp(self, epoch):
        z = (epoch - (self.end_epoch + self.start_epoch) / 2) / ((self.end_epoch - self.start_epoch) / 12)
        return self.max_kl_beta / (1.0 + math.exp(-z))
