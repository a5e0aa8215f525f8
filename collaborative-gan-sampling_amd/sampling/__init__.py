"""The reference's sampler classes (sampling/*.py), same names and call signatures."""
from .policy import PolicyAdaptive
from .rejector import Rejector
from .idpsampler import IndependenceSampler
from .device_rejector import DeviceRejector
from .device_idpsampler import DeviceIndependenceSampler
from . import collaborator, refiner_cpu

__all__ = ["PolicyAdaptive", "Rejector", "DeviceRejector", "IndependenceSampler", "DeviceIndependenceSampler", "collaborator", "refiner_cpu"]
