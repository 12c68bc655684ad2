"""Inputs of the encoder with a standardised input (EncoderPack(..., norm=(mean, std)); csrc/mlp_generic.hip, the NORM instantiation),
shared by tests/test_encode_std_norm_cpu.py and tests/test_gpu_encode_std_norm.py.  No GPU here.

The frames, labels, seeded models, recorded factors and the floor are those of tests/mlp_generic_cases.py; the bars and the float64
network those of tests/encode_ref.py, fed V = [xn32 | y].  The statistics are those of the fixture's first utterance (33 frames), by the
contract of dvae_frame_stats (tests/frame_stats_ref.py), so the other two utterances are not the pool they were taken from.  xn32 is
the float32 torch forms: the encoder's input by contract."""
import functools

import numpy as np

import encode_ref as ER
import frame_stats_ref as fs
import mlp_generic_cases as MC
import std_norm_cases as sc

NORM_EPS = sc.NORM_EPS


@functools.lru_cache(maxsize=None)
def stats():
    mean, std = fs.stats_ref(ER.power(MC.frames())[:MC.COUNTS[0]])
    return mean, std


def xn32():
    return sc.normalise(ER.power(MC.frames()), *stats(), NORM_EPS)


def inputs(labels):
    """V = [xn32 | y] float32"""
    return ER.inputs(xn32(), labels)
