"""Recipe for oracle/_ref/ (kept out of git): the reference's two driver scripts, byte-compiled as they are.

tests/test_host_logic.py executes the unmodified drivers (ego_pose/ego_mimic.py, ego_pose/ego_forecast.py) on the compat
packages. The tests run what build() leaves here, so they need no reference tree at test time; build() compiles them from
the first reference checkout it can read: $EGP_REFERENCE_DIR, a `reference` directory beside this repository, or the
default location /root/reference."""
import os
import py_compile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(REPO, "oracle", "_ref")
DRIVERS = ("ego_mimic", "ego_forecast")
REFERENCE_DIRS = (os.environ.get("EGP_REFERENCE_DIR"), os.path.join(os.path.dirname(REPO), "reference"), "/root/reference")


def compiled_driver(name):
    """Path of the compiled driver `name` (one of DRIVERS) in oracle/_ref/."""
    return os.path.join(REF_OUT, name + ".pyc")


def build():
    """Byte-compile the drivers into oracle/_ref/; returns the paths written (none without a readable reference tree)."""
    done = []
    for name in DRIVERS:
        src = next((s for s in (os.path.join(d, "ego_pose", name + ".py") for d in REFERENCE_DIRS if d) if os.access(s, os.R_OK)), None)
        if src is None:
            continue
        os.makedirs(REF_OUT, exist_ok=True)
        py_compile.compile(src, cfile=compiled_driver(name), dfile=name + ".py", doraise=True)
        done.append(compiled_driver(name))
    return done
