"""Generate tests/golden/kl_schedule.npz: the KL weights the UNMODIFIED reference schedules hand to `set_kl_beta`
(utils/callbacks/kl_callbacks.py KLLinearSchedule / KLSigmoidSchedule / KLConstantSchedule) for epochs 0..60 with the
arguments (start_epoch, end_epoch, max_kl_beta) = (10, 50, 0.1), recorded by driving each callback's own
on_train_epoch_start with a module stand-in that notes what it is given (needs the reference checkout that
oracle/ref_harness.py points at).

    python tools/gen_kl_schedule_golden.py

The fixture holds numbers only: epochs, args, linear (61), sigmoid (61), constant_calls (how often the constant schedule
called set_kl_beta: 0)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402

H.install_shims()
pl = sys.modules["pytorch_lightning"]
for name in ("Callback", "Trainer", "LightningModule"):  # names the module imports; only Callback is used, as a base class
    if not hasattr(pl, name):
        setattr(pl, name, type(name, (), {}))
for name in ("matplotlib", "matplotlib.pyplot"):  # imported at module level, used by its main() only
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
from tacorl.utils.callbacks import kl_callbacks as K  # noqa: E402

ARGS = (10, 50, 0.1)
EPOCHS = np.arange(61)


class _Module:
    def __init__(self):
        self.current_epoch, self.seen = 0, []

    def set_kl_beta(self, v):
        self.seen.append(v)


def record(cb):
    m = _Module()
    for e in EPOCHS:
        m.current_epoch = int(e)
        cb.on_train_epoch_start(None, m)
    return m.seen


def main():
    lin, sig, const = record(K.KLLinearSchedule(*ARGS)), record(K.KLSigmoidSchedule(*ARGS)), record(K.KLConstantSchedule())
    assert len(lin) == len(sig) == len(EPOCHS) and const == []
    path = os.path.join(ROOT, "tests", "golden", "kl_schedule.npz")
    np.savez_compressed(path, epochs=EPOCHS, args=np.array(ARGS), linear=np.array(lin, np.float64), sigmoid=np.array(sig, np.float64),
                        constant_calls=np.array(len(const)))
    print("wrote", path, "linear", lin[9:12], lin[49:52], "sigmoid", sig[9:12], sig[49:52])


if __name__ == "__main__":
    main()
