#!/opt/conda/bin/python3.9
"""HDF5 fixtures written by the REAL h5py / libhdf5 (this container only: /opt/conda/bin/python3.9 carries
h5py 3.3.0 on HDF5 1.10.6; the image's main interpreter and the GPU box have none).

What is written under tests/golden/hdf5/ (data only):

  deepconn_train.hdf5   the Tiny dataset's train split in the reference's quick-data layout: the 8 datasets
  narre_train.hdf5      a..h created exactly as data_scripts/make_quick_data.py:21-32 creates them (i8 / f8,
                        maxshape = shape, compression="gzip") and filled the way :34-44 fills them -- one sliced
                        assignment per loader batch, ragged last batch included.  The batches are the reference
                        loader's own (tests/golden/tiny/<mt>_streams.npz, produced by make_golden_tiny.py from
                        the reference's data.py).
  variants.hdf5         what else libhdf5 may hand a reader of such files: a contiguous (uncompressed) dataset,
                        gzip + shuffle, gzip + fletcher32, a dataset of 175 small chunks (a two-level chunk
                        B-tree), a dataset only partly written (absent chunks read as the fill value), a
                        non-zero fill value, f4 / i4 / big-endian types, more than 8 links in the root group
                        (several symbol-table nodes) and a nested group.
  expected.npz          the arrays h5py reads back from those files (the reader's known answers)
  random_<seed>.hdf5    h5py's own choices on random shapes, chunkings and filters (seeds 1, 2, 3): twelve datasets
                        of 1-3 dimensions, plain / chunked / gzip / gzip + shuffle at level 9 / fletcher32, and
                        'deep', 5,000 chunks of one row (a chunk B-tree three levels deep)
  random_expected.npz   the arrays h5py wrote into them, keyed '<file>/<dataset>'
  latest.hdf5           a file of libver='latest' (a layout the reader refuses by name)
  writer_checked.json   the other direction: hdf5_lite.write_file's files of sample_arrays() in three forms,
                        each opened by h5py (every dataset, dtype, shape, maxshape, compression, a slice) and walked
                        by libhdf5's h5ls before its size and sha256 were recorded

Usage:  /opt/conda/bin/python3.9 tests/golden/make_golden_hdf5.py
"""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import h5py
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'hdf5')
KEYS = 'abcdefgh'


def quick_file(mt, name):
    z = np.load(os.path.join(HERE, 'tiny', '%s_streams.npz' % mt))
    nb = 1 + max(int(k.split('/')[1]) for k in z.files if k.startswith('train/') and k.split('/')[1].isdigit())
    batches = [[z['train/%d/%s' % (b, s)] for s in ('0', '1', '2', '3', '4', '5', '6', 'y')] for b in range(nb)]
    n = sum(len(b[0]) for b in batches)
    shape = [n] + list(batches[0][0].shape[1:])
    path = os.path.join(OUT, name)
    with h5py.File(path, 'w') as f:
        dset = {}
        dset['a'] = f.create_dataset('a', shape, dtype='i8', maxshape=shape, compression='gzip')
        dset['b'] = f.create_dataset('b', [n, 10], dtype='i8', maxshape=[n, 10], compression='gzip')
        dset['c'] = f.create_dataset('c', [n, 10], dtype='i8', maxshape=[n, 10], compression='gzip')
        dset['d'] = f.create_dataset('d', shape, dtype='i8', maxshape=shape, compression='gzip')
        dset['e'] = f.create_dataset('e', shape, dtype='i8', maxshape=shape, compression='gzip')
        dset['f'] = f.create_dataset('f', [n], dtype='i8', maxshape=[n], compression='gzip')
        dset['g'] = f.create_dataset('g', [n], dtype='i8', maxshape=[n], compression='gzip')
        dset['h'] = f.create_dataset('h', [n], dtype='f8', maxshape=[n], compression='gzip')
        at = 0
        for fields in batches:
            bsz = len(fields[0])
            for k, v in zip(KEYS, fields):
                dset[k][at:at + bsz] = v
            at += bsz
    return path


def variants():
    rng = np.random.default_rng(20200725)
    path = os.path.join(OUT, 'variants.hdf5')
    with h5py.File(path, 'w') as f:
        f.create_dataset('contig', data=rng.integers(-2 ** 40, 2 ** 40, size=(13, 7), dtype=np.int64))
        f.create_dataset('shuf', data=rng.integers(0, 50000, size=(40, 33), dtype=np.int64), compression='gzip', shuffle=True)
        f.create_dataset('fletch', data=rng.standard_normal(301), compression='gzip', fletcher32=True)
        f.create_dataset('many', data=rng.integers(0, 1000, size=(700, 5), dtype=np.int64), chunks=(4, 5), compression='gzip')
        d = f.create_dataset('partial', (100, 6), dtype='i8', chunks=(16, 6), compression='gzip')
        d[40:56] = rng.integers(1, 99, size=(16, 6))
        d = f.create_dataset('filled', (9, 4), dtype='i8', chunks=(4, 4), fillvalue=-7)
        d[0:2] = 5
        f.create_dataset('f4', data=rng.standard_normal((6, 3)).astype(np.float32), compression='gzip')
        f.create_dataset('i4', data=rng.integers(-9, 9, size=17, dtype=np.int32))
        f.create_dataset('be', data=rng.integers(0, 2 ** 31, size=(5, 2)).astype('>i8'))
        f.create_dataset('edge', data=rng.integers(0, 9, size=(10, 7, 3), dtype=np.int64), chunks=(4, 4, 2), compression='gzip')
        f.create_dataset('empty', (0, 12), dtype='i8', maxshape=(0, 12), compression='gzip')
        g = f.create_group('grp')
        g.create_dataset('x', data=np.arange(11, dtype=np.float64))
    return path


def random_files():
    """random_<seed>.hdf5 + the arrays written into them; latest.hdf5."""
    exp = {}
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        name = 'random_%d.hdf5' % seed
        with h5py.File(os.path.join(OUT, name), 'w') as f:
            for i in range(12):
                nd = int(rng.integers(1, 4))
                shape = tuple(int(x) for x in rng.integers(1, 60, size=nd))
                chunks = tuple(int(rng.integers(1, s + 1)) for s in shape)
                dt = ['i8', 'f8', 'i4', 'f4', 'u2', 'i1'][int(rng.integers(0, 6))]
                a = (rng.standard_normal(shape) * 100).astype(dt)
                kw = [dict(), dict(chunks=chunks), dict(chunks=chunks, compression='gzip'),
                      dict(chunks=chunks, compression='gzip', shuffle=True, compression_opts=9),
                      dict(chunks=chunks, fletcher32=True)][int(rng.integers(0, 5))]
                f.create_dataset('d%d' % i, data=a, **kw)
                exp['%s/d%d' % (name, i)] = a
            a = rng.integers(0, 1 << 40, size=(5000, 3), dtype=np.int64)
            f.create_dataset('deep', data=a, chunks=(1, 3), compression='gzip')
            exp[name + '/deep'] = a
    np.savez_compressed(os.path.join(OUT, 'random_expected.npz'), **exp)
    with h5py.File(os.path.join(OUT, 'latest.hdf5'), 'w', libver='latest') as f:
        f.create_dataset('a', data=np.arange(10), chunks=(5,), compression='gzip')


def sample_arrays(seed=7, n=1000):
    """The arrays tests/test_hdf5_lite.py writes (its _sample_arrays)."""
    rng = np.random.default_rng(seed)
    return {'a': rng.integers(0, 50000, size=(n, 37)), 'b': rng.integers(0, 9, size=(n, 10)), 'h': rng.random(n) * 5,
            'f4': rng.random((7, 3)).astype(np.float32), 'e0': np.zeros((0, 12), np.int64),
            'u2': rng.integers(0, 60000, size=(33, 2, 3)).astype(np.uint16), 'i1': rng.integers(-9, 9, size=5).astype(np.int8)}


WRITER_FORMS = {'w0.hdf5': {}, 'w1.hdf5': {'chunk_bytes': 296}, 'w2.hdf5': {'compression': None}}


def writer_checked():
    """hdf5_lite.write_file's three forms of sample_arrays(), read by h5py and h5ls -> their sizes and sha256."""
    spec = importlib.util.spec_from_file_location(
        'hdf5_lite', os.path.join(HERE, '..', '..', 'reviews4rec_amd', 'hdf5_lite.py'))
    hdf5_lite = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hdf5_lite)
    exp = sample_arrays()
    out = {}
    tmp = tempfile.mkdtemp(prefix='r4r_h5w_')
    for fn, kw in WRITER_FORMS.items():
        path = os.path.join(tmp, fn)
        hdf5_lite.write_file(path, exp, **kw)
        with h5py.File(path, 'r') as f:
            assert sorted(f.keys()) == sorted(exp)
            assert len(f['a']) == 1000
            for k in exp:
                assert f[k].dtype == exp[k].dtype and f[k].shape == exp[k].shape and f[k].maxshape == exp[k].shape
                assert np.array_equal(f[k][:], exp[k]), (fn, k)
            assert np.array_equal(f['a'][200:400], exp['a'][200:400])
            assert (f['a'].compression == 'gzip' and f['a'].compression_opts == 4) if fn != 'w2.hdf5' else f['a'].chunks is None
        r = subprocess.run([os.path.join(os.path.dirname(sys.executable), 'h5ls'), '-r', '-v', path],
                           capture_output=True, text=True)
        assert r.returncode == 0 and 'Dataset {1000/1000, 37/37}' in r.stdout, r.stdout + r.stderr
        raw = open(path, 'rb').read()
        out[fn] = {'write_file_kwargs': kw, 'bytes': len(raw), 'sha256': hashlib.sha256(raw).hexdigest()}
    json.dump(out, open(os.path.join(OUT, 'writer_checked.json'), 'w'), indent=1)


def main():
    os.makedirs(OUT, exist_ok=True)
    expected = {}
    for mt, name in (('deepconn', 'deepconn_train.hdf5'), ('NARRE', 'narre_train.hdf5')):
        with h5py.File(quick_file(mt, name), 'r') as f:
            for k in KEYS:
                expected['%s/%s' % (name, k)] = f[k][:]
    with h5py.File(variants(), 'r') as f:
        for k in ('contig', 'shuf', 'fletch', 'many', 'partial', 'filled', 'f4', 'i4', 'edge', 'empty', 'grp/x'):
            expected['variants.hdf5/' + k] = f[k][:]
        expected['variants.hdf5/be'] = f['be'][:].astype(np.int64)      # (values; the file keeps them big-endian)
    np.savez_compressed(os.path.join(OUT, 'expected.npz'), **expected)
    random_files()
    writer_checked()
    for fn in sorted(os.listdir(OUT)):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == '__main__':
    main()
