"""Builds the stand-alone host checkers under tools/ (the device's source compiled as host C++, each with its own main) for the
tests that run them as child processes, with or without AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found for the host checker")


def build(tool_name, out_dir, sanitize, extra_flags=()):
    """tools/<tool_name>.cpp -> <out_dir>/<tool_name>, the program's path."""
    exe = os.path.join(str(out_dir), tool_name)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([compiler(), "-std=c++17", *flags, *extra_flags, os.path.join(ROOT, "tools", tool_name + ".cpp"), "-o", exe], check=True)
    return exe
