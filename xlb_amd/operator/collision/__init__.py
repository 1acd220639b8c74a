"""Collision operators of the HIP backend: BGK, KBC, Smagorinsky LES BGK, regularised BGK (projected and recursive)."""

from .collision import Collision as Collision, BGK as BGK, KBC as KBC, SmagorinskyLESBGK as SmagorinskyLESBGK
from .collision import RegularizedBGK as RegularizedBGK, RecursiveRegularizedBGK as RecursiveRegularizedBGK
