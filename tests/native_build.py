"""The native callers under tests/native that have a make file of their own (<name>.mk; __graft_entry__.build() runs each).  A
test that starts one asks for it here, so that a tests directory without build products - a fresh copy put beside an already
built library - still finds its program: make builds what is missing or older than its sources and does nothing otherwise."""
import os
import subprocess

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def caller(name):
    """Path of tests/native/<name>, built from <name>.mk if it is not there or out of date."""
    subprocess.check_call(["make", "-C", NATIVE, "-f", name + ".mk"], stdout=subprocess.DEVNULL)
    return os.path.join(NATIVE, name)
