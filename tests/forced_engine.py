"""An engine with some of its switches forced, for the GPU tests that run a picture through a form the engine would not choose.
An engine reads the OHEVC_* variables once, when it is created (openhevc_amd/csrc/engine_tuning.h), so the variables are set
around the creation only and the test's own process goes on with the environment it had."""
import contextlib
import os

SWITCHES = ("OHEVC_INTRA_MODE", "OHEVC_INTRA_WAVES", "OHEVC_INTRA_PHASES", "OHEVC_INTRA_RES_LDS", "OHEVC_COPY_THREADS")


@contextlib.contextmanager
def forced_engine(**switches):
    """with forced_engine(OHEVC_INTRA_MODE="dag") as eng: ...  -- Engine(0) created with exactly these of SWITCHES set"""
    assert set(switches) <= set(SWITCHES), switches
    from openhevc_amd.engine import Engine
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ.update({k: str(v) for k, v in switches.items()})
        eng = Engine(0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        yield eng
    finally:
        eng.close()
