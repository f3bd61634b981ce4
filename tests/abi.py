"""Shared helpers of the C-ABI tests (test_abi.py and the test_*_abi.py files): include/ofdis.h as text, its constants, the
library's export list and the two idioms of every argument-check test.  A plain module like common.py: no fixtures."""
import functools
import re
import subprocess

from of_dis_amd import capi
from of_dis_amd.abi import HEADER_PATH

NOT_NUMBERS = {"OFDIS_H_"}  # the include guard: the only #define without a value


@functools.lru_cache(maxsize=None)
def header():
    return open(HEADER_PATH).read()


def section(start, end):
    """the header from the first occurrence of `start` to the first occurrence of `end`"""
    hdr = header()
    return hdr[hdr.index(start):hdr.index(end)]


def _number(name, text):
    for pattern, value in ((r"\(1 << (\d+)\)", lambda s: 1 << int(s)), (r"(0x[0-9A-Fa-f]+|\d+)u?", lambda s: int(s, 0)),
                           (r"(\d+\.\d*)f?", float)):
        m = re.fullmatch(pattern, text)
        if m:
            return value(m.group(1))
    raise ValueError(f"include/ofdis.h: #define {name} {text}: not a number this parser knows")


@functools.lru_cache(maxsize=None)
def defines():
    """name -> value of every numeric #define, in header order"""
    found = re.findall(r"^#define[ \t]+(\w+)[ \t]*(.*?)[ \t]*(?:/\*.*)?$", header(), re.M)
    return {name: _number(name, text) for name, text in found if name not in NOT_NUMBERS}


@functools.lru_cache(maxsize=None)
def enumerators():
    """name -> value of every enumerator, in header order"""
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    return {name: int(value) for name, value in re.findall(r"\b(OFDIS_[A-Z0-9_]+)\s*=\s*(-?\d+)", code)}


def define(name):
    return defines()[name]


def enumerator(name):
    return enumerators()[name]


@functools.lru_cache(maxsize=None)
def exported():
    """the dynamic symbols the shipped library defines"""
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def rejected(rc, word=None):
    """the call returned OFDIS_ERR_INVALID and left a message, which names `word` if one is given"""
    assert rc == capi.ERR_INVALID
    msg = capi.lib().ofdis_last_error().decode()
    assert msg and (word is None or word in msg), (word, msg)


def ptr(array, on=True):
    """the address of a numpy array, or NULL"""
    return array.ctypes.data if on else None
