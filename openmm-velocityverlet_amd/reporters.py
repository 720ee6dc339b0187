"""Reporters for OpenMM's ``app.Simulation`` on top of the integrator's device-side services.

``DrudeTemperatureReporter`` writes the file that examples/ommhelper/reporter/drudetemperaturereporter.py writes -- the same header,
the same tab-separated columns (step, T_COM, T_Atom, T_Drude, KE_COM, KE_Atom, KE_Drude) -- but takes the numbers from
``simulation.integrator.getDrudeTemperatures()`` (computed on the GPU, 56 bytes copied back) instead of downloading every velocity
and looping over molecules and pairs on the host.  It asks OpenMM for no state at all.

``write_drude_temperature_series`` / ``write_viscosity_series`` write the rows of a device-side series (``Context.series_read``,
``distributed.drude_temperature_series``) into the files that reporter and examples/ommhelper/reporter/viscosityreporter.py write:
the same header and columns, one line per row, so that a long graph run keeps its sampled observables without stopping the GPU
for every sample.

``CheckpointReporter`` is examples/ommhelper/reporter/checkpointreporter.py on ``context.createCheckpoint()``: a file per report, the
latest three kept.

``write_dcd_frames`` writes the frames of a device-side recorder (``Context.frames_read``) as a DCD trajectory, what
``DCDReporter('dump.dcd', 10000)`` leaves behind for the same steps.

``write_profile`` writes a device-side density / velocity profile (``Context.profile_read``) as text columns, one line per bin.

``write_msd`` writes a device-side mean-squared displacement table (``Context.msd_read``) as text columns, one line per lag.

``write_vanhove`` writes a device-side self van Hove table (``Context.vanhove_read``) as text columns, one line per lag.

``write_vanhove_distinct`` writes one class of a device-side distinct van Hove table (``Context.vanhove_distinct_read``) as text columns, one line per bin.

``write_rdf`` writes device-side radial distribution functions (``Context.rdf_read``) as text columns, one line per bin.

``write_sdf`` writes one class of a device-side spatial distribution function (``Context.sdf_read``) as text, one line per non-zero voxel;
``write_sdf_cube`` writes it as a Gaussian cube file for isosurface viewers.

``write_current`` writes a device-side collective current correlation table (``Context.current_read``) as text columns, one line per lag.

``write_modes`` writes device-side density-mode correlations (``Context.modes_read``), S(k) and F(k, t), as text columns, one line per mode.

``write_contacts`` writes device-side contact lifetime correlations (``Context.contacts_read``) as text columns, one line per lag.

``write_acf`` writes device-side velocity or orientation autocorrelations (``Context.acf_read``) as text columns, one line per lag.

``write_cm_motion_record`` appends what the device-side removal of the centre-of-mass motion has done so far (``Context.cm_motion_record``).
"""
from __future__ import annotations

import os
import struct

import numpy as np

HEADER = '#"Step"\t"T_COM"\t"T_Atom"\t"T_Drude"\t"KE_COM"\t"KE_Atom"\t"KE_Drude"'
CM_MOTION_HEADER = '#"Step"\t"Removals"\t"Skipped"\t"Vx (nm/ps)"\t"Vy (nm/ps)"\t"Vz (nm/ps)"'
BOHR_NM = 0.0529177210903      # 1 bohr in nm (CODATA 2018): cube files carry lengths in bohr
VISCOSITY_HEADER ='#"Step"\t"Acceleration (nm/ps^2)"\t"VelocityAmplitude (nm/ps)"\t"1/Viscosity (1/Pa.s)"'
# 1/viscosity as the integrator returns it, in nm ps / (Da item), to 1/(Pa s): 1 Da nm^-1 ps^-1 = 1e18 / N_A Pa s
INV_VISCOSITY_TO_PER_PA_S = 6.02214076e23 * 1e-18


def _plain(x, unit_name):
    """A float from a plain number or an openmm.unit Quantity (the SWIG method returns Quantities in kJ/mol and K)."""
    if hasattr(x, "value_in_unit"):
        from openmm import unit
        return float(x.value_in_unit(getattr(unit, unit_name)))
    return float(x)


class DrudeTemperatureReporter:
    """Reports the temperatures of the molecules' centres of mass, of the atoms inside them and of the Drude pairs' relative
    motion every `reportInterval` steps.

    Parameters
    ----------
    file : str
        The file to write to
    reportInterval : int
        The interval (in time steps) at which to write a line
    append : bool
        Whether to append to an existing file
    """

    def __init__(self, file, reportInterval, append=False):
        self._reportInterval = int(reportInterval)
        self._out = open(file, "a" if append else "w")
        self._hasInitialized = False

    def describeNextReport(self, simulation):
        """(steps until the next report, positions?, velocities?, forces?, energies?): nothing is needed from the State."""
        steps = self._reportInterval - simulation.currentStep % self._reportInterval
        return (steps, False, False, False, False)

    def report(self, simulation, state):
        ke_com, ke_atom, ke_drude, t_com, t_atom, t_drude = simulation.integrator.getDrudeTemperatures()
        if not self._hasInitialized:
            print(HEADER, file=self._out)
            self._hasInitialized = True
        ke = [_plain(x, "kilojoule_per_mole") for x in (ke_com, ke_atom, ke_drude)]
        t = [_plain(x, "kelvin") for x in (t_com, t_atom, t_drude)]
        print(simulation.currentStep, *t, *ke, sep="\t", file=self._out)
        self._out.flush()

    def close(self):
        if self._out is not None and not self._out.closed:
            self._out.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CheckpointReporter:
    """Saves a checkpoint every `reportInterval` steps, as examples/ommhelper/reporter/checkpointreporter.py does: `file`_<step> holds
    ``simulation.context.createCheckpoint()`` of that step, and only the latest three files are kept.  (The reference's optional State
    XML next to it is not offered: there is no serializer here.)

    Parameters
    ----------
    file : str
        The file to write to; the step is appended to the name
    reportInterval : int
        The interval (in time steps) at which to write checkpoints
    """

    def __init__(self, file, reportInterval):
        if type(file) is not str:
            raise Exception("file should be str")
        self._file = file
        self._reportInterval = int(reportInterval)

    def describeNextReport(self, simulation):
        """(steps until the next report, positions?, velocities?, forces?, energies?): the checkpoint comes from the context itself."""
        steps = self._reportInterval - simulation.currentStep % self._reportInterval
        return (steps, False, False, False, False)

    def report(self, simulation, state):
        with open(self._file + "_%i" % simulation.currentStep, "wb") as out:
            out.write(simulation.context.createCheckpoint())
        prev3 = self._file + "_%i" % (simulation.currentStep - 3 * self._reportInterval)
        if os.path.exists(prev3):
            os.remove(prev3)


def _open(file, append):
    """(stream, close it afterwards?) for a path or an open text stream."""
    if hasattr(file, "write"):
        return file, False
    return open(file, "a" if append else "w"), True


def write_drude_temperature_series(file, series, append=False, header=True):
    """The rows of a series with its Drude part (Context.series_read) as DrudeTemperatureReporter writes them for the same steps and
    numbers: the header (unless header=False: a file continued from an earlier piece of the same run), then one tab-separated line
    (step, T_COM, T_Atom, T_Drude, KE_COM, KE_Atom, KE_Drude) per row.  `file`: a path or an open text stream."""
    if series.ke is None:
        raise ValueError("the series has no Drude part (series_start(drude=True))")
    out, own = _open(file, append)
    try:
        if header:
            print(HEADER, file=out)
        for j in range(len(series.step)):
            print(int(series.step[j]), *[float(x) for x in series.t[j]], *[float(x) for x in series.ke[j]], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def write_viscosity_series(file, series, append=False, header=True):
    """The rows of a series with its thermostat part as examples/ommhelper/reporter/viscosityreporter.py writes them: its header, then
    step, cos acceleration (nm/ps^2), velocity amplitude vMax (nm/ps) and 1/viscosity (1/(Pa s)) per row, tab-separated."""
    if series.v_max is None:
        raise ValueError("the series has no thermostat part (series_start(thermostat=True))")
    out, own = _open(file, append)
    try:
        if header:
            print(VISCOSITY_HEADER, file=out)
        for j in range(len(series.step)):
            print(int(series.step[j]), float(series.cos_acceleration[j]), float(series.v_max[j]),
                  float(series.inv_viscosity[j]) * INV_VISCOSITY_TO_PER_PA_S, sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def write_cm_motion_record(file, step, record, append=False, header=True):
    """One line for the record of the scheduled removals of the centre-of-mass motion (Context.cm_motion_record) as it stands at `step`:
    removals done, removals skipped, and the centre-of-mass velocity the last one subtracted."""
    out, own = _open(file, append)
    try:
        if header:
            print(CM_MOTION_HEADER, file=out)
        print(int(step), int(record.removals), int(record.skipped), *[float(x) for x in record.last_v], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def profile_columns(profile):
    """[(name, values per bin)] of a profile's text file: the bin centre, then per group the recorded quantities as sums over the samples."""
    cols = [("%s (nm)" % "xyz"[profile.axis], profile.centres)]
    for g in range(profile.words.shape[0]):
        cols.append(("count[%d]" % g, profile.count[g]))
        if profile.charge is not None:
            cols.append(("charge[%d] (e)" % g, profile.charge[g]))
        if profile.mass is not None:
            cols.append(("mass[%d] (Da)" % g, profile.mass[g]))
        if profile.momentum is not None:
            cols += [("p%s[%d] (Da nm/ps)" % ("xyz"[k], g), profile.momentum[g, k]) for k in range(3)]
        if profile.kinetic is not None:
            cols.append(("mv2[%d] (Da nm^2/ps^2)" % g, profile.kinetic[g]))
    return cols


def write_profile(file, profile, append=False, header=True):
    """A profile (Context.profile_read, distributed.profile_sum) as text: two comment lines (samples, dropped, out of range; the column
    names) unless header=False, then one tab-separated line per bin -- the bin centre, then per group the recorded quantities as summed
    over the samples (divide by `samples` and the bin volume for densities: Profile.number_density).  Floats are written with repr, so
    np.loadtxt reads back the bits.  `file`: a path or an open text stream."""
    cols = profile_columns(profile)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"OutOfRange"\t%d' % (profile.samples, profile.dropped, profile.out_of_range), file=out)
            print("#" + "\t".join('"%s"' % name for name, _ in cols), file=out)
        for b in range(len(profile.edges) - 1):
            print(*[repr(float(v[b])) for _, v in cols], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def msd_columns(msd, dt):
    """[(name, values per lag)] of an MSD's text file: the lag in ps, then per group the pairs, the total and x | y | z in nm^2."""
    cols = [("lag (ps)", msd.lag_steps.astype(np.float64) * float(dt))]
    values, total = msd.msd, msd.total
    for g in range(msd.words.shape[0]):
        cols.append(("pairs[%d]" % g, msd.pairs[g].astype(np.float64)))
        cols.append(("msd[%d] (nm^2)" % g, total[g]))
        cols += [("msd_%s[%d] (nm^2)" % ("xyz"[k], g), values[g, :, k]) for k in range(3)]
    return cols


def write_msd(file, msd, dt, append=False, header=True):
    """A mean-squared displacement table (Context.msd_read, distributed.msd_sum) as text: two comment lines (samples, dropped, out of
    range, origin floor; the column names) unless header=False, then one tab-separated line per lag -- the lag in ps (lag steps x `dt`),
    then per group the pairs, <|dr|^2> and <dx^2> | <dy^2> | <dz^2> in nm^2 (nan where a lag has no pairs).  Floats are written with repr,
    so np.loadtxt reads back the bits.  `file`: a path or an open text stream."""
    cols = msd_columns(msd, dt)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"OutOfRange"\t%d\t"OriginFloor"\t%d' % (msd.samples, msd.dropped, msd.out_of_range, msd.origin_floor), file=out)
            print("#" + "\t".join('"%s"' % name for name, _ in cols), file=out)
        for l in range(msd.words.shape[1]):
            print(*[repr(float(v[l])) for _, v in cols], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def vanhove_columns(vh, dt):
    """[(name, values per lag)] of a self van Hove table's text file: the lag in ps, then per group the pairs, below, beyond, <r^2>, <r^4>,
    alpha_2 and the probability of every bin."""
    cols = [("lag (ps)", vh.lag_steps.astype(np.float64) * float(dt))]
    msd, r4, alpha2, P = vh.msd, vh.r4, vh.alpha2, vh.P
    for g in range(vh.head.shape[0]):
        cols += [("%s[%d]" % (name, g), v[g].astype(np.float64)) for name, v in (("pairs", vh.pairs), ("below", vh.below), ("beyond", vh.beyond))]
        cols += [("msd[%d] (nm^2)" % g, msd[g]), ("r4[%d] (nm^4)" % g, r4[g]), ("alpha2[%d]" % g, alpha2[g])]
        cols += [("P[%d][%d]" % (g, b), P[g, :, b]) for b in range(vh.hist.shape[2])]
    return cols


def write_vanhove(file, vh, dt, append=False, header=True):
    """A self van Hove table (Context.vanhove_read, distributed.vanhove_sum) as text: three comment lines (samples, dropped, out of range,
    origin floor; the bin edges in nm; the column names) unless header=False, then one tab-separated line per lag -- the lag in ps (lag
    steps x `dt`), then per group the pairs, those below and beyond the bins, <r^2>, <r^4>, alpha_2 and the probability P of every bin
    (nan where a lag has no pairs; G_s is P divided by the shell volume of the edges).  Floats are written with repr, so np.loadtxt reads
    back the bits.  `file`: a path or an open text stream."""
    cols = vanhove_columns(vh, dt)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"OutOfRange"\t%d\t"OriginFloor"\t%d' % (vh.samples, vh.dropped, vh.out_of_range, vh.origin_floor), file=out)
            print('#"Edges (nm)"\t' + "\t".join(repr(float(e)) for e in vh.edges), file=out)
            print("#" + "\t".join('"%s"' % name for name, _ in cols), file=out)
        for l in range(vh.head.shape[1]):
            print(*[repr(float(v[l])) for _, v in cols], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def rdf_columns(rdf):
    """[(name, values per bin)] of an RDF's text file: the bin centre in nm, then per class the count, g(r) and the coordination number."""
    cols = [("r (nm)", rdf.r)]
    g, n = rdf.g(), rdf.coordination()
    for c in range(rdf.counts.shape[0]):
        tag = "%d-%d" % (int(rdf.classes[c, 0]), int(rdf.classes[c, 1]))
        cols += [("count[%s]" % tag, rdf.counts[c].astype(np.float64)), ("g[%s]" % tag, g[c]), ("n[%s]" % tag, n[c])]
    return cols


def write_rdf(file, rdf, append=False, header=True):
    """Radial distribution functions (Context.rdf_read) as text: two comment lines (samples, dropped, invalid, the sum of 1 / V; the
    column names) unless header=False, then one tab-separated line per bin -- the bin centre in nm, then per class the pair count, g(r)
    and the running coordination number.  Floats are written with repr, so np.loadtxt reads back the bits.  `file`: a path or an open
    text stream."""
    cols = rdf_columns(rdf)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"Invalid"\t%d\t"InvVolumeSum"\t%r' % (rdf.samples, rdf.dropped, rdf.invalid, float(rdf.inv_volume_sum)), file=out)
            print("#" + "\t".join('"%s"' % name for name, _ in cols), file=out)
        for b in range(rdf.counts.shape[1]):
            print(*[repr(float(v[b])) for _, v in cols], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def write_sdf(file, sdf, c=0, append=False, header=True):
    """One class of a spatial distribution function (Context.sdf_read) as text: two comment lines (samples, dropped, invalid, bad frames,
    the frame visits of the class's frame group, the sum of 1 / V, extent and voxels per axis; the column names) unless header=False, then
    one tab-separated line per NON-ZERO voxel in the table's order -- its three indices, its centre in nm along xi1, xi2, xi3, the count,
    the density in nm^-3 and g.  Floats are written with repr, so np.loadtxt reads back the bits.  `file`: a path or an open text stream."""
    x, rho, g = sdf.centres, sdf.density(c), sdf.g(c)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"Invalid"\t%d\t"BadFrames"\t%d\t"FrameVisits"\t%d\t"InvVolumeSum"\t%r\t"Extent (nm)"\t%r\t"Bins"\t%d\t"Class"\t"%d-%d"'
                  % (sdf.samples, sdf.dropped, sdf.invalid, sdf.bad_frames, int(sdf.frame_visits[sdf.classes[c, 0]]), float(sdf.inv_volume_sum),
                     float(sdf.extent), sdf.nbins, int(sdf.classes[c, 0]), int(sdf.classes[c, 1])), file=out)
            print("#" + "\t".join('"%s"' % name for name in ("i1", "i2", "i3", "xi1 (nm)", "xi2 (nm)", "xi3 (nm)", "count", "density (nm^-3)", "g")), file=out)
        for i, j, k in np.argwhere(sdf.counts[c] != 0):
            print(i, j, k, repr(float(x[i])), repr(float(x[j])), repr(float(x[k])), int(sdf.counts[c, i, j, k]), repr(float(rho[i, j, k])),
                  repr(float(g[i, j, k])), sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def write_sdf_cube(file, sdf, c=0, quantity="g"):
    """One class of a spatial distribution function as a Gaussian cube file, which VMD and similar viewers open as an isosurface:
    `quantity` is "g", "density" (nm^-3) or "counts".  Two comment lines; one atom record (a carbon, for the viewer's sake) at the frame's
    origin, which is the centre of the cube; the grid's origin at the first voxel's centre, (-h + voxel / 2) on every axis; the voxel
    vectors along xi1, xi2, xi3; lengths in bohr; the data in the table's own C order (xi1 outermost, xi3 fastest), six values per line,
    a new line after every xi3 run.  NaN (no visit, no sample) is written as 0."""
    n, step = sdf.nbins, sdf.voxel / BOHR_NM
    data = {"g": sdf.g, "density": sdf.density, "counts": lambda k: sdf.counts[k].astype(np.float64)}[quantity](c)
    data = np.where(np.isnan(data), 0.0, data)
    first = (-sdf.extent + 0.5 * sdf.voxel) / BOHR_NM
    out, own = _open(file, False)
    try:
        print("spatial distribution function, %s, class %d-%d (frame group - site group)" % (quantity, int(sdf.classes[c, 0]), int(sdf.classes[c, 1])), file=out)
        print("samples %d, frame visits %d, extent %r nm, axes xi1 xi2 xi3, lengths in bohr" % (sdf.samples, int(sdf.frame_visits[sdf.classes[c, 0]]), float(sdf.extent)), file=out)
        print("%5d %12.6f %12.6f %12.6f" % (1, first, first, first), file=out)
        for a in range(3):
            print("%5d %12.6f %12.6f %12.6f" % ((n,) + tuple(step if b == a else 0.0 for b in range(3))), file=out)
        print("%5d %12.6f %12.6f %12.6f %12.6f" % (6, 6.0, 0.0, 0.0, 0.0), file=out)
        for i in range(n):
            for j in range(n):
                row = data[i, j]
                for k0 in range(0, n, 6):
                    print(" ".join("%13.5E" % v for v in row[k0:k0 + 6]), file=out)
        out.flush()
    finally:
        if own:
            out.close()


def current_columns(cur, dt):
    """[(name, values per lag)] of a current table's text file: the lag in ps, the count, then per displacement class g <= h
    sum_a <dP_g,a dP_h,a> and per current class (g, h) sum_a <J_g,a(0) J_h,a(t)>."""
    cols = [("lag (ps)", cur.lag_steps.astype(np.float64) * float(dt)), ("count", cur.count.astype(np.float64))]
    G = cur.num_groups
    cols += [("disp[%d-%d] (e^2 nm^2)" % (g, h), cur.displacement(g, h).sum(axis=1)) for g in range(G) for h in range(g, G)]
    cols += [("cur[%d-%d] (e^2 nm^2/ps^2)" % (g, h), cur.correlation(g, h).sum(axis=1)) for g in range(G) for h in range(G)]
    return cols


def write_current(file, cur, dt, append=False, header=True):
    """A collective current correlation table (Context.current_read) as text: two comment lines (samples, dropped, out of range, invalid
    samples, origin floor, the sum of 1 / V; the column names) unless header=False, then one tab-separated line per lag from the zero lag
    on -- the lag in ps (lag steps x `dt`), the count of time origins, per pair of groups g <= h the mean product of the collective
    displacements summed over x, y, z, and per ordered pair (g, h) the mean product of the currents (nan where a lag has no origin).
    Floats are written with repr, so np.loadtxt reads back the bits.  `file`: a path or an open text stream."""
    cols = current_columns(cur, dt)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"OutOfRange"\t%d\t"InvalidSamples"\t%d\t"OriginFloor"\t%d\t"InvVolumeSum"\t%r' %
                  (cur.samples, cur.dropped, cur.out_of_range, cur.invalid_samples, cur.origin_floor, float(cur.inv_volume_sum)), file=out)
            print("#" + "\t".join('"%s"' % name for name, _ in cols), file=out)
        for l in range(cur.words.shape[0]):
            print(*[repr(float(v[l])) for _, v in cols], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def write_modes(file, dm, dt, g=0, h=0, append=False, header=True):
    """Density-mode correlations (Context.modes_read) as text: two comment lines (samples, dropped, out of range, invalid samples, origin
    floor, the box sums; the column names) unless header=False, then one tab-separated line per mode -- n_x, n_y, n_z, |k| in 1/nm from
    the mean box, S_gh(k), then F_gh(k, t) for every lag from the first on (the lag times in ps, lag steps x `dt`, are in the column
    names; nan where a lag has no origin).  Floats are written with repr, so np.loadtxt reads back the bits.  `file`: a path or an open
    text stream."""
    F = dm.F(g, h)
    k = dm.k_magnitudes()
    lags = dm.lag_steps.astype(np.float64) * float(dt)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"OutOfRange"\t%d\t"InvalidSamples"\t%d\t"OriginFloor"\t%d\t"BoxSum"\t%r\t%r\t%r' %
                  (dm.samples, dm.dropped, dm.out_of_range, dm.invalid_samples, dm.origin_floor, *[float(x) for x in dm.box_sum]), file=out)
            names = ["nx", "ny", "nz", "k (1/nm)", "S[%d-%d]" % (g, h)] + ["F[%d-%d](%r ps)" % (g, h, float(t)) for t in lags[1:]]
            print("#" + "\t".join('"%s"' % name for name in names), file=out)
        for m in range(F.shape[1]):
            print(*[str(int(c)) for c in dm.modes[m]], repr(float(k[m])), *[repr(float(v)) for v in F[:, m]], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def write_vanhove_distinct(file, vhd, dt, c=0, append=False, header=True):
    """One class of a distinct van Hove table (Context.vanhove_distinct_read) as text: three comment lines (samples, dropped, invalid,
    origin floor; per row the visits; the column names) unless header=False, then one tab-separated line per bin -- the bin centre in nm,
    then G_d of class `c` for every row from the zero lag on (the lag times in ps, lag steps x `dt`, are in the column names; nan where a
    row has no visit).  Floats are written with repr, so np.loadtxt reads back the bits.  `file`: a path or an open text stream."""
    G = vhd.G_d(c)
    r = vhd.r
    lags = vhd.lag_steps.astype(np.float64) * float(dt)
    tag = "%d-%d" % (int(vhd.classes[c, 0]), int(vhd.classes[c, 1]))
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"Invalid"\t%d\t"OriginFloor"\t%d' % (vhd.samples, vhd.dropped, vhd.invalid, vhd.origin_floor), file=out)
            print('#"Visits"\t' + "\t".join(str(int(v)) for v in vhd.visits), file=out)
            print("#" + "\t".join('"%s"' % name for name in ["r (nm)"] + ["G_d[%s](%r ps)" % (tag, float(t)) for t in lags]), file=out)
        for b in range(G.shape[1]):
            print(repr(float(r[b])), *[repr(float(v)) for v in G[:, b]], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def contacts_columns(con, dt):
    """[(name, values per lag)] of a contact table's text file: the lag in ps, the visits, then per class the contacts at the origin, those
    that are contacts again, those that never broke, and the two correlations C(t) and S(t)."""
    cols = [("lag (ps)", con.lag_steps.astype(np.float64) * float(dt)), ("origins", con.origins.astype(np.float64))]
    for c in range(con.words.shape[0]):
        tag = "%d-%d" % (int(con.classes[c, 0]), int(con.classes[c, 1]))
        cols += [("at_origin[%s]" % tag, con.words[c, :, 1].astype(np.float64)), ("again[%s]" % tag, con.words[c, :, 2].astype(np.float64)),
                 ("unbroken[%s]" % tag, con.words[c, :, 3].astype(np.float64)), ("C[%s]" % tag, con.intermittent(c))]
        if con.continuous_kept:
            cols.append(("S[%s]" % tag, con.continuous(c)))
    return cols


def write_contacts(file, con, dt, append=False, header=True):
    """Contact lifetime correlations (Context.contacts_read) as text: two comment lines (samples, dropped, invalid; the column names)
    unless header=False, then one tab-separated line per lag from the zero lag on -- the lag in ps (lag steps x `dt`), the count of
    (origin, sample) pairs, then per class the three contact counts (exact below 2^53), the intermittent correlation C(t) and, where the
    recorder kept it, the continuous one S(t) (nan where no origin had a contact).  Floats are written with repr, so np.loadtxt reads
    back the bits.  `file`: a path or an open text stream."""
    cols = contacts_columns(con, dt)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"Invalid"\t%d' % (con.samples, con.dropped, con.invalid), file=out)
            print("#" + "\t".join('"%s"' % name for name, _ in cols), file=out)
        for l in range(con.words.shape[1]):
            print(*[repr(float(v[l])) for _, v in cols], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


def acf_columns(acf, dt):
    """[(name, values per lag)] of an autocorrelation table's text file: the lag in ps, then per group the pairs and, in the velocity modes,
    C = <v(0).v(t)> with its three components, in orientation mode P1 and P2."""
    cols = [("lag (ps)", acf.lag_steps.astype(np.float64) * float(dt))]
    for g in range(acf.words.shape[0]):
        cols.append(("pairs[%d]" % g, acf.pairs[g].astype(np.float64)))
        if acf.mode == "orientation":
            cols += [("P1[%d]" % g, acf.P1(g)), ("P2[%d]" % g, acf.P2(g))]
        else:
            comp = acf.components(g)
            cols.append(("C[%d] (nm^2/ps^2)" % g, acf.C(g)))
            cols += [("C_%s[%d] (nm^2/ps^2)" % ("xyz"[k], g), comp[:, k]) for k in range(3)]
    return cols


def write_acf(file, acf, dt, append=False, header=True):
    """An autocorrelation table (Context.acf_read, distributed.acf_sum) as text: two comment lines (samples, dropped, out of range, origin
    floor; the column names) unless header=False, then one tab-separated line per lag from the zero lag on -- the lag in ps (lag steps x
    `dt`), then per group the pair count and the correlations (nan where a row has no pairs).  Floats are written with repr, so np.loadtxt
    reads back the bits.  `file`: a path or an open text stream."""
    cols = acf_columns(acf, dt)
    out, own = _open(file, append)
    try:
        if header:
            print('#"Samples"\t%d\t"Dropped"\t%d\t"OutOfRange"\t%d\t"OriginFloor"\t%d' % (acf.samples, acf.dropped, acf.out_of_range, acf.origin_floor), file=out)
            print("#" + "\t".join('"%s"' % name for name, _ in cols), file=out)
        for l in range(acf.words.shape[1]):
            print(*[repr(float(v[l])) for _, v in cols], sep="\t", file=out)
        out.flush()
    finally:
        if own:
            out.close()


DCD_TITLE = (b"Created by openmm-velocityverlet_amd", b"")


def _dcd_step_interval(first, count, interval, steps):
    """The header's step interval after `steps` follow `count` frames that began at `first` with `interval`: their common distance, 0 when
    the steps are not equidistant (or there is one frame only)."""
    steps = [int(x) for x in steps]
    if count == 0:
        first, count, steps = steps[0], 1, steps[1:]
        interval = steps[0] - first if steps else 0
    elif count == 1:
        interval = steps[0] - first if steps else 0
    if interval <= 0:
        return 0
    return interval if all(x == first + interval * (count + j) for j, x in enumerate(steps)) else 0


def write_dcd_frames(file, frames, dt, append=False):
    """The frames of a device-side recorder (Context.frames_read) as a DCD trajectory at `file` (a path).  `dt`: the step size in ps.

    Little-endian Fortran-unformatted records, each framed by its int32 byte count in front and behind:
      * 84 bytes: ``CORD``; nine int32 -- number of frames, first step, step interval (0 when the steps are not equidistant, as on a
        logarithmic schedule), six zeros; float32 dt; int32 1 (a unit cell per frame); eight int32 zeros; int32 24;
      * 164 bytes: int32 2 and two title lines of 80 bytes;
      * 4 bytes: the number of atoms;
      * per frame 48 bytes of six float64 ``a, 0, b, 0, 0, c`` in Angstrom (the zeros: the cosines of the 90 degree angles), then three
        records of m float32: x, y and z in Angstrom, nm x 10 multiplied in float32.
    This is the layout OpenMM's DCDFile writes as far as it is documented and remembered; there is no OpenMM here to compare a file with,
    so it is NOT pinned against one (OpenMM puts the date into the title, this writer does not: equal frames give equal bytes).
    append=True adds the frames to a file this function wrote and rewrites the header's frame count (byte offset 8) and step interval
    (byte offset 16): a file written in pieces equals the file written at once.  Positions are written as recorded: unwrapped."""
    if frames.positions is None:
        raise ValueError("the frames hold no positions (frames_start(positions=True))")
    n, m = len(frames.step), len(frames.particles)
    pos = np.asarray(frames.positions).astype(np.float32, copy=False) * np.float32(10)
    cell = np.zeros((n, 6), dtype="<f8")
    cell[:, 0], cell[:, 2], cell[:, 5] = frames.box[:, 0] * 10.0, frames.box[:, 1] * 10.0, frames.box[:, 2] * 10.0

    def record(payload):
        return struct.pack("<i", len(payload)) + payload + struct.pack("<i", len(payload))

    body = bytearray()
    for j in range(n):
        body += record(cell[j].tobytes())
        for k in range(3):
            body += record(np.ascontiguousarray(pos[j, :, k], dtype="<f4").tobytes())
    if append:
        with open(file, "r+b") as out:
            head = out.read(24)
            if len(head) < 24 or head[:8] != struct.pack("<i", 84) + b"CORD":
                raise ValueError(f"{file} is no DCD file of this writer")
            count, first, interval = struct.unpack("<3i", head[8:20])
            out.seek(4 + 84 + 4 + 4 + 164 + 4 + 4)
            if struct.unpack("<i", out.read(4))[0] != m:
                raise ValueError(f"{file} holds frames of another number of atoms")
            if n:
                new_first = first if count else int(frames.step[0])
                new_interval = _dcd_step_interval(first, count, interval, frames.step)
                out.seek(8)
                out.write(struct.pack("<3i", count + n, new_first, new_interval))
                out.seek(0, os.SEEK_END)
                out.write(body)
        return
    first = int(frames.step[0]) if n else 0
    interval = _dcd_step_interval(0, 0, 0, frames.step) if n else 0
    head = b"CORD" + struct.pack("<9i", n, first, interval, *([0] * 6)) + struct.pack("<f", float(dt)) + struct.pack("<i", 1) + \
        struct.pack("<8i", *([0] * 8)) + struct.pack("<i", 24)
    title = struct.pack("<i", len(DCD_TITLE)) + b"".join(line.ljust(80)[:80] for line in DCD_TITLE)
    with open(file, "wb") as out:
        out.write(record(head) + record(title) + record(struct.pack("<i", m)) + bytes(body))
