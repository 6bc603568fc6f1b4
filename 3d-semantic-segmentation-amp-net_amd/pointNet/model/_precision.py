"""The `precision` attribute of the modules that launch kernels, in a module of its own so that pointnetAtt.py (which imports the
PointNet++ blocks) and pointnet2_utils.py can both take it without importing each other."""
from ... import _lib


class _HasPrecision:
    """Mix-in of the modules that launch kernels: `precision` is the matrix precision every C-ABI call made on the module's behalf runs
    in (_lib.precision_scope), None = follow the library's process-wide default.  A forward in grad mode records the mode it ran in and
    its backward runs in that mode (autograd.py), so changing the attribute between the two does not touch a step under way."""
    precision = None

    def set_precision(self, mode):
        self.precision = None if mode is None else _lib.checked_precision(mode)
        return self


def is_bf16(mode):
    """True for the names of the bf16 forward mode ('bf16', 'bfloat16'); None and the fp32 names are False."""
    return mode is not None and _lib.PRECISIONS[mode] == _lib.PRECISIONS["bf16"]


class _EvalForwardPrecision(_HasPrecision):
    """_HasPrecision for the PointNet++ modules, whose kernels do not consult the library's mode: `precision` names the ENTRY POINTS the
    eval forward without a graph goes through.  None and the fp32 names ('fp32', 'f32', 'float32') are the exact-fp32 kernels whatever
    the process-wide mode, a precision scope or AMPNET_PRECISION says (for the other models None follows the library's default: a
    deliberate difference); 'bf16' / 'bfloat16' are the bf16 forwards, an inference mode that a module built for gradients, batch
    statistics or a whole-cloud group refuses (_bf16_refusal: the reason, or None); the remaining modes are not built."""

    def _bf16_refusal(self):
        raise NotImplementedError

    def set_precision(self, mode):
        mode = None if mode is None else _lib.checked_precision(mode)
        name = type(self).__name__
        if is_bf16(mode):
            why = self._bf16_refusal()
            if why:
                raise NotImplementedError(f"{name}: precision={mode!r} is the eval forward without a graph (inference); {why}")
        elif mode is not None and _lib.PRECISIONS[mode] != _lib.PRECISIONS["fp32"]:
            raise NotImplementedError(f"{name}: precision={mode!r} is not built; built are 'fp32' (None: exact fp32, the default) and 'bf16' "
                                      f"(the eval forward without a graph)")
        self.precision = mode
        return self

    def _check_bf16(self):
        """Every forward: a flag set on the module after construction does not turn a bf16 module into an fp32 one silently."""
        if is_bf16(self.precision):
            self.set_precision(self.precision)
