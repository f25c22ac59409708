"""ERA5 loader surface of the reference (utils/data_loader_era5.py:21-181) feeding SYNTHETIC Gaussian fields.

`get_data_loader(params, files_pattern, distributed, train)` returns `(loader, dataset, sampler)` for training and
`(loader, dataset)` otherwise, with the reference's tensor contract:
    inp [B, n_in, H, W], tar [B, n_out*(n_future+1), H, W]  (+ zen_inp [B,1,H,W], zen_tar [B,n_future+1,H,W] if add_zenith)
and the reference's dataset index arithmetic (year / local index, year-boundary wrap :158-160, target slab :164-165).
Data sources, in the order `get_data_loader` tries them:
  * year files under `files_pattern` (`*.npy` memmaps, fp32 or int16-packed by utils/pack_dataset.py, or `*.h5` with h5py -- the
    reference's format) -> the host pipeline of
    utils/host_pipeline.py: pinned staging ring, async H2D, crop / z-score / zenith / invariants assembled by HIP kernels;
  * `params.synthetic_host_samples > 0`: the same pipeline over an in-memory synthetic year array (PCIe-inclusive benchmarks);
  * `params.synthetic_device_pool > 0` (default of the bench configs): `DevicePoolLoader`, K batches generated ON THE DEVICE once
    and cycled, so the timed loop has no host RNG and no H2D copy (605 MB / sample binds a step to PCIe otherwise);
  * otherwise a torch DataLoader over the synthetic `GetDataset` (CPU generation; plumbing / tests): each "year file" is a
    virtual array fields[N, 73, 721, 1440] of iid N(0,1) values that is a pure function of (seed, year, time index), cropped to
    img_size like :163-165 and normalised with means 0 / stds 1.
Real data is used whenever it is found; the synthetic sources are explicit params flags (no silent fallback when a data path
was given but holds no files: that raises).
"""
import logging
import math

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler


def worker_init(wrk_id):
    np.random.seed(torch.utils.data.get_worker_info().seed % (2 ** 32 - 1))


def is_leap_year(yr):
    return (yr % 4 == 0)


def _get(params, key, default):
    return params[key] if key in params else default


def sun_position(year: int, hours: float):
    """(sin dec, cos dec, hour angle at longitude 0) of the Sun `hours` after Jan 1st 00:00 UTC of `year`, float64 scalars.

    The time-dependent part of the reference's zenith channel (data_loader_era5.py:109-146 -> modulus.utils.zenith_angle.
    cos_zenith_angle, a dependency that is absent here): Greenwich mean sidereal time (IAU-82 polynomial), the Sun's true
    ecliptic longitude (mean longitude + equation of centre), obliquity, then right ascension / declination;
    hour angle(lon) = GMST + lon - RA.  Everything that varies per pixel is left to cos_zenith / the HIP kernel:
    cos(zenith) = sin(lat) sin(dec) + cos(lat) cos(dec) cos(hour angle).  oracle/zenith.py restates the published routine
    function by function; tests hold this implementation to it."""
    import datetime
    t = datetime.datetime(int(year), 1, 1) + datetime.timedelta(hours=float(hours)) - datetime.datetime(2000, 1, 1, 12)
    jc = (t.days + t.seconds / 86400.0 + t.microseconds / 86400.0e6) / 36525.0           # Julian centuries since J2000.0
    gmst = math.radians((67310.54841 + jc * (876600 * 3600 + 8640184.812866 + jc * (0.093104 - jc * 6.2 * 10e-6))) / 240.0) % (2 * math.pi)
    m = math.radians(357.52910 + 35999.05030 * jc - 0.0001559 * jc * jc - 0.00000048 * jc ** 3)
    lam = math.radians(280.46645 + 36000.76983 * jc + 0.0003032 * jc * jc) + math.radians(
        (1.914600 - 0.004817 * jc - 0.000014 * jc * jc) * math.sin(m) + (0.019993 - 0.000101 * jc) * math.sin(2 * m) + 0.000290 * math.sin(3 * m))
    eps = math.radians(23.0 + 26.0 / 60 + 21.406 / 3600.0 - (46.836769 * jc - 0.0001831 * jc ** 2 + 0.00200340 * jc ** 3
                                                            - 0.576e-6 * jc ** 4 - 4.34e-8 * jc ** 5) / 3600.0)
    x, y, z = math.cos(lam), math.cos(eps) * math.sin(lam), math.sin(eps) * math.sin(lam)
    r = math.sqrt(1.0 - z * z)
    dec, ra = math.atan2(z, r), 2.0 * math.atan2(y, x + r)
    ha0 = math.remainder(gmst - ra, 2 * math.pi)            # reduced in float64: the kernel adds the longitude in fp32
    return math.sin(dec), math.cos(dec), ha0


def cos_zenith(year: int, hours: float, H: int, W: int) -> torch.Tensor:
    """cos of the solar zenith angle on the 0.25-degree grid (lat 90 .. -90, lon 0 .. 359.75; data_loader_era5.py:60-64),
    [H, W] float32 (rows cropped like :175-176), `hours` after Jan 1st of `year` (:127-131)."""
    sd, cd, ha0 = sun_position(year, hours)
    lat = torch.deg2rad(torch.linspace(90.0, -90.0, 721, dtype=torch.float64)[:H]).view(-1, 1)
    lon = torch.deg2rad(torch.arange(0, 360, 0.25, dtype=torch.float64)[:W]).view(1, -1)
    return (torch.sin(lat) * sd + torch.cos(lat) * cd * torch.cos(ha0 + lon)).float()


class GetDataset(Dataset):
    def __init__(self, params, location, train):
        self.params, self.location, self.train = params, location, train
        self.dt = params.dt
        self.in_channels = np.asarray(params.in_channels)
        self.out_channels = np.asarray(params.out_channels)
        self.n_in_channels = params.n_in_channels
        self.n_out_channels = params.n_out_channels
        self.n_future = params.n_future
        self.seed = _get(params, 'seed', None) or 333          # data_loader_era5_dali.py:100 default
        self.n_years = _get(params, 'synthetic_n_years', 2)
        self.years = [1979 + i for i in range(self.n_years)] if train else [2016 + i for i in range(self.n_years)]
        self.n_samples_per_year = _get(params, 'synthetic_samples_per_year', 1460)
        self.img_shape_x, self.img_shape_y = params.img_size[0], params.img_size[1]
        assert self.img_shape_x <= 721 and self.img_shape_y <= 1440, 'image shapes are greater than dataset image shapes'
        self.n_samples_total = self.n_years * self.n_samples_per_year
        logging.info("Synthetic ERA5: {} virtual years x {} samples, image {} x {} x {}".format(
            self.n_years, self.n_samples_per_year, self.img_shape_x, self.img_shape_y, self.n_in_channels))

    def __len__(self):
        return self.n_samples_total

    def _fields(self, year_idx, t, channels):
        """rows `channels` of the virtual fields[t] of year `year_idx`, cropped: [len(channels), H, W] N(0,1)"""
        g = torch.Generator().manual_seed((self.seed * 1000003 + self.years[year_idx]) * 10007 + int(t))
        full = torch.randn(73, self.img_shape_x, self.img_shape_y, generator=g)
        return full[torch.as_tensor(channels)]

    def index(self, global_idx):
        """year / local index with the reference's boundary handling (:149-160)"""
        year_idx = int(global_idx / self.n_samples_per_year)
        local_idx = int(global_idx % self.n_samples_per_year)
        step = self.dt
        local_idx = local_idx % (self.n_samples_per_year - step * (self.n_future + 1))
        if local_idx < step:
            local_idx += step
        return year_idx, local_idx

    def __getitem__(self, global_idx):
        year_idx, local_idx = self.index(global_idx)
        step = self.dt
        inp = self._fields(year_idx, local_idx, self.in_channels)
        tar = torch.stack([self._fields(year_idx, t, self.out_channels)
                           for t in range(local_idx + step, local_idx + step * (self.n_future + 1) + 1, step)], 0)
        tar = tar.reshape(self.n_out_channels * (self.n_future + 1), self.img_shape_x, self.img_shape_y)
        if self.params.add_zenith:
            H, W = self.img_shape_x, self.img_shape_y
            zi = cos_zenith(self.years[year_idx], 6.0 * local_idx, H, W).unsqueeze(0)
            zt = torch.stack([cos_zenith(self.years[year_idx], 6.0 * t, H, W)
                              for t in range(local_idx + step, local_idx + step * (self.n_future + 1) + 1, step)], 0)
            return inp, tar, zi, zt
        return inp, tar


class DevicePoolLoader:
    """K device-resident batches, generated once with the device RNG (seed = base seed + rank) and cycled.  With a zenith channel /
    static features (configs with `add_zenith`, `add_orography`, `add_landmask`) the pool holds the batches as the host pipeline delivers
    them: the model's input already ASSEMBLED in one buffer -- [data channels | cos zenith | land mask (2) | orography] in the
    reference's order (preprocess_utils.py:50-68) -- so the PreProcessor passes them through instead of concatenating 319 MB per sample
    in every step (the 375 us CatArrayBatchedCopy of round 4's cfg-4 profile); `assemble=False` keeps the raw tuples."""

    def __init__(self, params, dataset, device, train, pool, steps_per_epoch, assemble=True):
        self.dataset, self.steps, self.batches = dataset, steps_per_epoch, []
        B, H, W = int(params.local_batch_size), dataset.img_shape_x, dataset.img_shape_y
        n_in = len(dataset.in_channels)
        n_tar = dataset.n_out_channels * (dataset.n_future + 1)
        g = torch.Generator(device=device).manual_seed(dataset.seed + 7919 * _get(params, 'data_shard_id', 0) + (0 if train else 1))
        stat = None
        if assemble and (_get(params, 'add_orography', False) or _get(params, 'add_landmask', False)):
            from .preprocess_utils import build_static_features
            stat = build_static_features(params)
            stat = None if stat is None else stat.to(device)
        for k in range(pool):
            inp = torch.randn(B, n_in, H, W, device=device, generator=g)
            tar = torch.randn(B, n_tar, H, W, device=device, generator=g)
            zi = zt = None
            if params.add_zenith:
                zi = cos_zenith(dataset.years[0], 6.0 * k, H, W).to(device).expand(B, 1, H, W).contiguous()
                zt = torch.stack([cos_zenith(dataset.years[0], 6.0 * (k + 1 + s), H, W) for s in range(dataset.n_future + 1)],
                                 0).to(device).unsqueeze(0).expand(B, -1, H, W).contiguous()
            if assemble and (zi is not None or stat is not None):
                from .host_pipeline import AssembledBatch
                parts = [inp] + ([zi] if zi is not None else []) + ([stat.expand(B, -1, -1, -1)] if stat is not None else [])
                self.batches.append(AssembledBatch((torch.cat(parts, dim=1).contiguous(), tar, zt)))       # once, at pool creation
            elif zi is not None:
                self.batches.append((inp, tar, zi, zt))
            else:
                self.batches.append((inp, tar))

    def __len__(self):
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            yield self.batches[i % len(self.batches)]


def _year_files(location):
    import glob
    import os
    loc = str(location or '')
    return os.path.isdir(loc) and (glob.glob(os.path.join(loc, '*.npy')) or glob.glob(os.path.join(loc, '*.h5')))


class _PipelineDataset:
    """the attributes train.py reads from `dataset` (img_shape_x / _y, n_samples) for a pipeline-backed loader"""

    def __init__(self, pipe):
        self.img_shape_x, self.img_shape_y = pipe.H, pipe.W
        self.n_samples_total = pipe.n_total
        self.n_in_channels = pipe.n_in

    def __len__(self):
        return self.n_samples_total


def get_data_loader(params, files_pattern, distributed, train):
    host_n = _get(params, 'synthetic_host_samples', 0)
    if _year_files(files_pattern) or host_n:
        from .host_pipeline import Era5HostPipeline, SyntheticYearSource
        from .packed import open_year_source
        from .preprocess_utils import build_static_features
        device = torch.device('cuda', torch.cuda.current_device())
        if _year_files(files_pattern):
            source = open_year_source(str(files_pattern))       # int16-packed .npy files (utils/packed.py) or the fp32 year files
        else:
            source = SyntheticYearSource(n_years=1, n_samples=int(host_n), seed=_get(params, 'seed', None) or 333,
                                         pinned=bool(_get(params, 'synthetic_host_pinned', False)))
        stat = build_static_features(params)
        pipe = Era5HostPipeline(params, source, device, train, static_features=None if stat is None else stat[0],
                                steps_per_epoch=_get(params, 'synthetic_steps_per_epoch', None))
        ds = _PipelineDataset(pipe)
        return (pipe, ds, pipe) if train else (pipe, ds)      # the pipeline is its own "sampler" (set_epoch)
    if _get(params, 'require_data_files', False):
        raise FileNotFoundError(f"no year files (*.npy / *.h5) under {files_pattern!r} and require_data_files is set")
    dataset = GetDataset(params, files_pattern, train)
    pool = _get(params, 'synthetic_device_pool', 0)
    if pool:
        device = torch.device('cuda', torch.cuda.current_device())
        shards = _get(params, 'data_num_shards', 1)
        steps = _get(params, 'synthetic_steps_per_epoch', max(1, len(dataset) // (int(params.local_batch_size) * shards)))
        loader = DevicePoolLoader(params, dataset, device, train, pool, steps)
        return (loader, dataset, None) if train else (loader, dataset)
    sampler = DistributedSampler(dataset, shuffle=train, num_replicas=params.data_num_shards,
                                 rank=params.data_shard_id) if distributed else None
    dataloader = DataLoader(dataset, batch_size=int(params.local_batch_size), num_workers=params.num_data_workers,
                            shuffle=(sampler is None), sampler=sampler, worker_init_fn=worker_init, drop_last=True,
                            pin_memory=torch.cuda.is_available())
    return (dataloader, dataset, sampler) if train else (dataloader, dataset)
