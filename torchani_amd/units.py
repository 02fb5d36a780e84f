"""Unit conversions with the public names of the reference's ``torchani.units``.

The constants are the CODATA 2014 values (the ones ASE 3.x uses): the Hartree in eV, the elementary charge, Avogadro's
number, the atomic mass unit and the speed of light; the calorie and the metric prefixes are exact.  The vibrational factors
turn the square root of an eigenvalue of a mass-scaled Hessian (Hartree / (amu Angstrom^2)) into a wavenumber or an energy,
and an eigenvalue into a force constant in mDyne / Angstrom.
"""
from __future__ import annotations

import math

ANGSTROM_TO_BOHR = 1.8897261258369282        # 1 / Bohr radius in Angstrom, as ase.units.Bohr derives it from CODATA 2014
HARTREE_TO_EV = 27.211386024367243           # (CODATA 2014, as ase.units.Hartree)
EV_TO_JOULE = 1.6021766208e-19               # elementary charge in C (CODATA 2014)
JOULE_TO_KCAL = 1.0 / 4184.0                 # thermochemical calorie (exact)
HARTREE_TO_JOULE = HARTREE_TO_EV * EV_TO_JOULE
AVOGADROS_NUMBER = 6.022140857e23            # 1 / mol (CODATA 2014)
SPEED_OF_LIGHT = 299792458.0                 # m / s (exact)
AMU_TO_KG = 1.660539040e-27                  # kg (CODATA 2014)
ANGSTROM_TO_METER = 1e-10
NEWTON_TO_MILLIDYNE = 1e8                    # 1 N = 1e5 dyne = 1e8 mDyne
HARTREE_TO_KCALPERMOL = HARTREE_TO_JOULE * JOULE_TO_KCAL * AVOGADROS_NUMBER
HARTREE_TO_KJOULEPERMOL = HARTREE_TO_JOULE * AVOGADROS_NUMBER / 1000
# energy density Hartree / Angstrom^3 -> GPa (elastic constants, stress)
HARTREE_PER_ANGSTROM3_TO_GPA = HARTREE_TO_JOULE / ANGSTROM_TO_METER ** 3 / 1e9
EV_TO_KCALPERMOL = EV_TO_JOULE * JOULE_TO_KCAL * AVOGADROS_NUMBER
EV_TO_KJOULEPERMOL = EV_TO_JOULE * AVOGADROS_NUMBER / 1000
DEBYE_TO_ELECTRON_ANGSTROM = 0.2081943       # 1 D = 0.2081943 e Angstrom
# 1 cm^-1 in eV: h c 100 / e
INVCM_TO_EV = 6.626070040e-34 * SPEED_OF_LIGHT * 100.0 / EV_TO_JOULE
# sqrt(Hartree / (amu Angstrom^2)) is an angular frequency in 1/s once the energy is in J, the mass in kg and the length in m;
# divided by c (m/s) and by 100 it is a wavenumber in cm^-1 (~17092)
SQRT_MHESSIAN_TO_INVCM = math.sqrt(HARTREE_TO_JOULE / AMU_TO_KG) / ANGSTROM_TO_METER / SPEED_OF_LIGHT / 100.0
SQRT_MHESSIAN_TO_MILLIEV = SQRT_MHESSIAN_TO_INVCM * INVCM_TO_EV * 1000.0
# Hartree / Angstrom^2 -> mDyne / Angstrom (~4.36)
MHESSIAN_TO_FCONST = HARTREE_TO_JOULE * NEWTON_TO_MILLIDYNE / ANGSTROM_TO_METER
# thermal conductivity from a Green-Kubo integral in the units of the MD engine: J in Hartree Angstrom / fs, V in Angstrom^3,
# t in fs and k_B in Hartree / K (md.KB_HARTREE) give  1 / (3 V k_B T^2) int <J(0) . J(t)> dt  in Hartree / (Angstrom fs K).
# With the CODATA 2018 Hartree of md.ACC_UNIT, 1 Ha = 4.3597447222071e-18 J, 1 Angstrom = 1e-10 m and 1 fs = 1e-15 s:
# 1 Ha / (Angstrom fs K) = 4.3597447222071e-18 J / (1e-10 m 1e-15 s K) = 4.3597447222071e7 W / (m K)
HARTREE_PER_ANGSTROM_FS_KELVIN_TO_WATT_PER_METER_KELVIN = 4.3597447222071e-18 / (1e-10 * 1e-15)

# older names of the reference
HARTREE_TO_KCALMOL = HARTREE_TO_KCALPERMOL
EV_TO_KCALMOL = EV_TO_KCALPERMOL
HARTREE_TO_KJOULEMOL = HARTREE_TO_KJOULEPERMOL
EV_TO_KJOULEMOL = EV_TO_KJOULEPERMOL


def angstrom2bohr(x):
    return x * ANGSTROM_TO_BOHR


def bohr2angstrom(x):
    return x / ANGSTROM_TO_BOHR


def sqrt_mhessian2invcm(x):
    """sqrt of a mass-scaled Hessian eigenvalue (sqrt(Hartree / (amu Angstrom^2))) -> cm^-1."""
    return x * SQRT_MHESSIAN_TO_INVCM


def sqrt_mhessian2milliev(x):
    """sqrt of a mass-scaled Hessian eigenvalue -> meV."""
    return x * SQRT_MHESSIAN_TO_MILLIEV


def mhessian2fconst(x):
    """Hessian eigenvalue (Hartree / (amu Angstrom^2)) times amu -> mDyne / Angstrom."""
    return x * MHESSIAN_TO_FCONST


def hartree2ev(x):
    return x * HARTREE_TO_EV


def ev2kjoulepermol(x):
    return x * EV_TO_KJOULEPERMOL


def ev2kcalpermol(x):
    return x * EV_TO_KCALPERMOL


def hartree2kjoulepermol(x):
    return x * HARTREE_TO_KJOULEPERMOL


def hartree2kcalpermol(x):
    return x * HARTREE_TO_KCALPERMOL


def ea2debye(x):
    """Dipole in e Angstrom -> Debye."""
    return x / DEBYE_TO_ELECTRON_ANGSTROM


def hartree_per_angstrom3_to_gpa(x):
    return x * HARTREE_PER_ANGSTROM3_TO_GPA


# older names of the reference
hartree2kcalmol = hartree2kcalpermol
hartree2kjoulemol = hartree2kjoulepermol
ev2kcalmol = ev2kcalpermol
ev2kjoulemol = ev2kjoulepermol
