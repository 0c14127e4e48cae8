"""What the CPU suites of the Python and C faces share (a helper module; no pytest settings): the loaded library, the fixture that
refuses it, and a host tensor that claims to be on the device.  A suite takes the fixture with `from _faces import no_library`:
pytest finds a fixture in the importing module's namespace."""
import pytest
import torch


def lib():
    from lsdradixsort_amd import lib

    return lib()


@pytest.fixture
def no_library(monkeypatch):
    """The argument checks come first: the library must not even be asked for."""
    import lsdradixsort_amd as lsd

    def refuse():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(lsd.api, "lib", refuse)
    return lsd


class FakeCuda(torch.Tensor):
    """a host tensor whose is_cuda is True: it passes the wrappers' device check, so the checks after it can be reached"""
    is_cuda = True
