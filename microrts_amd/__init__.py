"""microrts_amd — MI355X-native vectorised microRTS env step (HIP kernels behind a C ABI).

Drop-in for tests.JNIGridnetVecClient of the reference (src/tests/JNIGridnetVecClient.java).
"""
from .vec_client import JNIGridnetVecClient, UnitTypeTable  # noqa: F401
from .device_env import DeviceVecEnv  # noqa: F401
from .forward_model import ForwardModel  # noqa: F401
from .policy_head import evaluate_actions, evaluate_actions_packed  # noqa: F401

__all__ = ["JNIGridnetVecClient", "UnitTypeTable", "DeviceVecEnv", "ForwardModel", "evaluate_actions", "evaluate_actions_packed"]
