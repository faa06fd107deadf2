"""The geometry and the mixed gensteps shared by test_gensteps.py (host twin)
and test_gpu_gensteps.py (device): tests/scenes.py materials plus one
dispersive material, n rising linearly from 1.33 at 300 nm to 1.36 at 600 nm."""
import numpy as np

from chroma import gensteps as gs
from chroma import make
from chroma.detector import Detector
from chroma.geometry import Material, Solid, standard_wavelengths

import scenes


def dispersive_material():
    m = Material('dispersive')
    wl = standard_wavelengths.astype(np.float64)
    m.set('refractive_index', 1.33 + 0.03 * np.clip((wl - 300.0) / 300.0, 0.0, 1.0))
    m.set('absorption_length', 1e6)
    m.set('scattering_length', 1e6)
    return m


def build():
    """(geometry, PackedGeometry, dict of Material objects)."""
    from chroma import loader
    from chroma.gpu.packing import PackedGeometry
    m = scenes.materials()
    m['disp'] = dispersive_material()
    det = Detector(m['water'])
    det.add_solid(Solid(make.box(2000.0, 2000.0, 2000.0), m['water'], m['water']))
    det.add_solid(Solid(make.box(300.0, 300.0, 300.0), m['scint'], m['water']), displacement=(0, 0, -500))
    det.add_solid(Solid(make.box(300.0, 300.0, 300.0), m['disp'], m['water']), displacement=(0, 0, 500))
    geo = loader.create_geometry_from_obj(det)
    return geo, PackedGeometry(geo), m


X0, DX, T0, DT = (10.0, 20.0, 30.0), (100.0, -50.0, 25.0), 5.0, 2.0
MIXED_COUNTS = (0, 1, 63, 64, 65, 1000, 0, 777, 300)


def mixed_steps(m):
    """Steps of MIXED_COUNTS photons: small ones of every kind around the wave
    size, empty ones, 1000 scintillation, 777 Cherenkov, 300 isotropic."""
    kw = dict(x0=X0, dx=DX, t0=T0, dt=DT)
    parts = [gs.isotropic_flash(m['water'], 0, evidx=0, **kw),
             gs.cherenkov_step(m['disp'], 1, beta=0.9, wavelength_range=(300.0, 600.0), evidx=1, **kw),
             gs.isotropic_flash(m['water'], 63, wavelength_range=(300.0, 600.0), evidx=2, **kw),
             gs.scintillation_step(m['scint'], 64, component=1, evidx=3, **kw),
             gs.cherenkov_step(m['water'], 65, beta=0.8, wavelength_range=(250.0, 650.0), evidx=4, **kw),
             gs.scintillation_step(m['scint'], 1000, component=0, evidx=5, **kw),
             gs.cherenkov_step(m['disp'], 0, beta=0.9, wavelength_range=(300.0, 600.0), evidx=6, **kw),
             gs.cherenkov_step(m['disp'], 777, beta=0.9, wavelength_range=(300.0, 600.0), evidx=7, **kw),
             gs.isotropic_flash(m['water'], 300, evidx=8, **kw)]
    steps = gs.Gensteps.join(parts)
    assert tuple(steps.steps['nphotons']) == MIXED_COUNTS
    return steps
