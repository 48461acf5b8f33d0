"""Host-side mirror of the reference's Seq driver (py/sequence.py) on top of the C-ABI.

Names and argument meaning follow the reference so tests read like its code:

    reference (py/sequence.py)                      here
    ------------------------------------------      -------------------------------------------
    get_reference_seqs(paths)            :189-194   Sequencer.get_reference_seqs(paths)
    mdf_generator(f)                     :197-221   Sequencer.batch_from_mdf(text) (parsed in C++)
    mdf_to_seq(mdf, targets)             :303-320   Sequencer.mdf_to_seq(molecules, target, ...)
    perfect / badread                    :242-270   target="perfect" / "badread"
    fastq_formatter / fasta_formatter    :273-288   fastq=True / False
    Identities / ErrorModel / QScoreModel           set_identity / load_error_model / load_qscore_model

All arithmetic happens in libtksmseq.so (HIP kernels); nothing here computes sequence data.
"""
import ctypes as C

import numpy as np

from . import _lib as L

# the empty member that ends a BGZF file (SAM specification 4.1.2); tksmseq_gzip_eof returns the same 28 bytes
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class TksmSeqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"tksmseq error {code}: {msg}")
        self.code = code


class Batch:
    def __init__(self, seq, handle):
        self._seq, self._h = seq, handle
        n, ni, nm = C.c_uint64(), C.c_uint64(), C.c_uint64()
        seq._lib.tksmseq_batch_info(handle, C.byref(n), C.byref(ni), C.byref(nm))
        self.n_reads, self.n_intervals, self.n_mods = n.value, ni.value, nm.value

    def free(self):
        if self._h:
            self._seq._lib.tksmseq_batch_free(self._seq._ctx, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RunResult:
    def __init__(self, seq, res):
        self._seq = seq
        self.records_ptr, self.offsets_ptr = res.records, res.record_offsets
        self.records_bytes, self.n_reads = res.records_bytes, res.n_reads
        self.bases_in, self.bases_out = res.bases_in, res.bases_out
        self.kernel_ms = list(res.kernel_ms)

    def download(self):
        rec = np.empty(self.records_bytes, np.uint8)
        off = np.empty(self.n_reads + 1, np.uint64)
        self._seq._chk(self._seq._lib.tksmseq_result_download(self._seq._ctx, rec.ctypes.data, off.ctypes.data))
        return rec.tobytes(), off

    def download_range(self, offset, nbytes):
        """bytes [offset, offset + nbytes) of the record stream (tksmseq_result_download_range)"""
        rec = np.empty(nbytes, np.uint8)
        self._seq._chk(self._seq._lib.tksmseq_result_download_range(self._seq._ctx, rec.ctypes.data, offset, nbytes, 0))
        return rec.tobytes()

    def copy_to_device(self, records_ptr=None, offsets_ptr=None):
        self._seq._chk(self._seq._lib.tksmseq_result_copy_device(
            self._seq._ctx, C.c_void_p(records_ptr) if records_ptr else None, C.c_void_p(offsets_ptr) if offsets_ptr else None))

    def records(self):
        rec, off = self.download()
        return [rec[int(off[i]):int(off[i + 1])] for i in range(self.n_reads)]

    def gzip(self, with_info=False):
        """The records as BGZF members compressed on the device (tksmseq_result_gzip): bytes that every gzip reader reads; members
        of several batches concatenate, a file ends with BGZF_EOF.  with_info: (bytes, member offsets u64[n + 1], device ms)."""
        g = L.GzipResult()
        self._seq._chk(self._seq._lib.tksmseq_result_gzip(self._seq._ctx, C.byref(g)))
        return self._seq._gzip_fetch(g, with_info)

    def stats(self):
        ist = np.empty((self.n_reads, 16), np.int32)
        dst = np.empty((self.n_reads, 2), np.float64)
        self._seq._chk(self._seq._lib.tksmseq_stats_download(self._seq._ctx, ist.ctypes.data, dst.ctypes.data))
        return ist, dst


class TranscribePlan:
    """One abundance table joined with the Sequencer's transcript table (tksmseq_transcribe_plan_create): .rows data rows, .records
    emitted rows, .molecules the sum of their depths, .missing the ids the GTFs lack, in row order."""

    def __init__(self, seq, handle):
        self._seq, self._h = seq, handle
        v = [C.c_uint64() for _ in range(4)]
        seq._lib.tksmseq_transcribe_plan_info(handle, *[C.byref(x) for x in v])
        self.rows, self.records, self.molecules, n_missing = [x.value for x in v]
        self.missing = []
        for i in range(n_missing):
            p, n = C.c_void_p(), C.c_uint64()
            seq._lib.tksmseq_transcribe_plan_missing(handle, i, C.byref(p), C.byref(n))
            self.missing.append(C.string_at(p, n.value).decode())

    def batch(self, first=0, n=None, comments=True):
        """molecules [first, first + n) of the unrolled records as a batch on the device (tksmseq_transcribe); n None: all from first"""
        n = max(0, self.molecules - first) if n is None else n
        h = C.c_void_p()
        self._seq._chk(self._seq._lib.tksmseq_transcribe(self._seq._ctx, self._h, int(first), int(n), 0 if comments else L.MOL_NO_COMMENTS, C.byref(h)))
        return Batch(self._seq, h)

    def mdf_text(self, first_record=0, n_records=None):
        """the reference's own output: one record per emitted row with depth = its count (tksmseq_transcribe_text)"""
        t, n = C.c_void_p(), C.c_uint64()
        self._seq._chk(self._seq._lib.tksmseq_transcribe_text(self._h, int(first_record), self.records if n_records is None else int(n_records),
                                                               C.byref(t), C.byref(n)))
        try:
            return C.string_at(t, n.value).decode()
        finally:
            self._seq._lib.tksmseq_text_free(t)

    def close(self):
        if self._h:
            self._seq._lib.tksmseq_transcribe_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Targets:
    """The transcripts of the Sequencer's table spliced from its reference on the device (tksmseq_targets_from_transcripts; the rules in
    include/tksmseq.h, "map, annotated targets"): .info the counters of tksmseq_targets_info, .names, .lengths, .voff and .projectable per
    target.  Pass it to Sequencer.map(targets=...).  Stale once the reference or the transcript table of the Sequencer changes; free it
    before the Sequencer is closed."""

    def __init__(self, seq, handle, info):
        self._seq, self._h = seq, handle
        self.info = {n: getattr(info, n) for n, _ in L.TargetsInfo._fields_ if n != "reserved"}
        self.names, self.lengths, self.voff, self.projectable = [], [], [], []
        name, ln, voff, proj = C.c_char_p(), C.c_uint32(), C.c_uint64(), C.c_int32()
        for t in range(info.targets):
            seq._lib.tksmseq_targets_get(handle, t, C.byref(name), C.byref(ln), C.byref(voff), C.byref(proj))
            self.names.append(name.value.decode())
            self.lengths.append(ln.value)
            self.voff.append(voff.value)
            self.projectable.append(bool(proj.value))

    def download(self):
        """(codes, valid): the image as uint32 arrays of 2 * image_vwords and image_vwords words"""
        n = self.info["image_vwords"]
        codes, valid = np.empty(2 * n, np.uint32), np.empty(n, np.uint32)
        self._seq._chk(self._seq._lib.tksmseq_targets_download(self._seq._ctx, self._h, codes.ctypes.data, valid.ctypes.data))
        return codes, valid

    def write_fasta(self, path, line_width=60):
        """the targets as a FASTA (.gz: compressed on the host), N for a letter outside ACGT; line_width 0: one line a target"""
        self._seq._chk(self._seq._lib.tksmseq_targets_write_fasta(self._seq._ctx, self._h, str(path).encode(), int(line_width)))

    def free(self):
        if self._h:
            self._seq._lib.tksmseq_targets_free(self._seq._ctx, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Variants:
    """A variant table in its normal form (tksmseq_variants_load): .rows lines read, of which .snvs, .insertions and .deletions; the
    deletions' union is .deleted_ranges disjoint ranges, and .dropped_points SNVs / insertions lie inside one.  Host only; may be used
    with any Sequencer."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        v = [C.c_uint64() for _ in range(6)]
        lib.tksmseq_variants_info(handle, *[C.byref(x) for x in v])
        self.rows, self.snvs, self.insertions, self.deletions, self.deleted_ranges, self.dropped_points = [x.value for x in v]

    def close(self):
        if self._h:
            self._lib.tksmseq_variants_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sequencer:
    """One context = one GPU (the reference's module globals: reference_seqs, identities, models).

    Several contexts in flight (clone(), one host thread and stream each) want a hardware queue each: start the process with
    GPU_MAX_HW_QUEUES=16 in its environment (read once, when the HIP runtime starts; its default of 4 makes the streams of different
    contexts share queues, and their kernels then run one after the other).  The `tksm` CLI and bench.py set it for their own
    processes; importing this module does not touch the embedding application's environment."""

    def __init__(self, device=0, stream=None):
        self._lib = L.load()
        ctx = C.c_void_p()
        rc = self._lib.tksmseq_create(device, C.byref(ctx))
        if rc:
            raise TksmSeqError(rc, self._lib.tksmseq_last_error(None).decode())
        self._ctx = ctx
        if stream is not None:
            self._chk(self._lib.tksmseq_set_stream(self._ctx, C.c_void_p(stream)))

    def clone(self, stream=None):
        """A second Sequencer on the same device that shares this one's packed reference and model tables (for another
        host thread / batch in flight).  Close clones before the source.  (Hardware queues: GPU_MAX_HW_QUEUES=16, see the class.)"""
        other = object.__new__(Sequencer)
        other._lib = self._lib
        ctx = C.c_void_p()
        self._chk(self._lib.tksmseq_clone(self._ctx, C.byref(ctx)))
        other._ctx = ctx
        other._parent = self          # keeps the source alive
        if stream is not None:
            other._chk(self._lib.tksmseq_set_stream(other._ctx, C.c_void_p(stream)))
        return other

    def close(self):
        if self._ctx:
            self._lib.tksmseq_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise TksmSeqError(rc, self._lib.tksmseq_last_error(self._ctx).decode())

    # ---- reference
    def get_reference_seqs(self, paths):
        for p in paths:
            self._chk(self._lib.tksmseq_reference_add_fasta(self._ctx, str(p).encode()))

    def add_contig(self, name, seq):
        """seq: bytes/str (host) or an object with data_ptr()/numel() holding ASCII bytes on this GPU."""
        if hasattr(seq, "data_ptr"):
            self._chk(self._lib.tksmseq_reference_add_contig(self._ctx, name.encode(), C.c_void_p(seq.data_ptr()),
                                                             seq.numel(), 1))
        else:
            b = seq.encode() if isinstance(seq, str) else bytes(seq)
            buf = (C.c_char * len(b)).from_buffer_copy(b) if len(b) else None
            self._chk(self._lib.tksmseq_reference_add_contig(self._ctx, name.encode(),
                                                             C.cast(buf, C.c_void_p) if buf is not None else None, len(b), 0))

    def declare_contig(self, name, length):
        """a contig known by name and length only, as `<reference>.fai` lists it (tksmseq_reference_declare_contig): enough for wgs()
        and to_mdf_text(); run() on such a context fails"""
        self._chk(self._lib.tksmseq_reference_declare_contig(self._ctx, name.encode(), int(length)))

    def contig_id(self, name):
        return self._lib.tksmseq_reference_contig_id(self._ctx, name.encode())

    def reference_info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._lib.tksmseq_reference_info(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return {"n_contigs": a.value, "total_bases": b.value, "device_bytes": c.value}

    # ---- models
    def load_error_model(self, name_or_path):
        self._chk(self._lib.tksmseq_load_error_model(self._ctx, str(name_or_path).encode()))

    def load_qscore_model(self, name_or_path):
        self._chk(self._lib.tksmseq_load_qscore_model(self._ctx, str(name_or_path).encode()))

    def load_tail_model(self, name_or_path="no_noise"):
        """KDE_noise_generator.load (py/tksm_badread.py:944-962); "no_noise" switches the tail off."""
        self._chk(self._lib.tksmseq_load_tail_model(self._ctx, str(name_or_path).encode()))

    def set_tail_model(self, lx, ly, grid, trans, ratio, bases="AGTC"):
        """The same from arrays (KDE_noise_generator.__init__, py/tksm_badread.py:905-917)."""
        lx = np.ascontiguousarray(lx, np.float64); ly = np.ascontiguousarray(ly, np.float64)
        grid = np.ascontiguousarray(grid, np.float64); trans = np.ascontiguousarray(trans, np.float64)
        if grid.shape != (len(ly), len(lx)) or trans.shape != (4, 4) or len(bases) != 4:
            raise ValueError("tail model: grid must be len(ly) x len(lx), trans 4 x 4, bases 4 symbols")
        b = bases.encode() if isinstance(bases, str) else bytes(bases)
        d = L.TailModelDesc(len(lx), len(ly), lx.ctypes.data, ly.ctypes.data, grid.ctypes.data, (C.c_double * 16)(*trans.ravel()),
                          float(ratio), (C.c_uint8 * 4)(*b), (C.c_uint8 * 4)())
        self._chk(self._lib.tksmseq_set_tail_model(self._ctx, C.byref(d)))

    def set_identity(self, mean=84.0, max_identity=99.0, stdev=5.5):
        self._chk(self._lib.tksmseq_set_identity(self._ctx, mean, max_identity, stdev))

    def error_model_tables(self):
        t, k, a = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._lib.tksmseq_get_error_model(self._ctx, C.byref(t), C.byref(k), C.byref(a), None, None, None))
        n = 4 ** k.value
        cdf, alts, nalts = np.empty((n, a.value), np.uint32), np.empty((n, a.value), np.uint64), np.empty(n, np.uint8)
        self._chk(self._lib.tksmseq_get_error_model(self._ctx, None, None, None, cdf.ctypes.data, alts.ctypes.data,
                                                    nalts.ctypes.data))
        return {"type": t.value, "k": k.value, "max_alts": a.value, "cdf": cdf, "alts": alts, "nalts": nalts}

    def qscore_model_tables(self):
        ns, ks, pl = C.c_int32(), C.c_int32(), C.c_uint64()
        self._chk(self._lib.tksmseq_get_qscore_model(self._ctx, C.byref(ns), C.byref(ks), C.byref(pl), None, None, None,
                                                     None, None))
        keys, off, cnt = np.empty(ns.value, np.uint64), np.empty(ns.value, np.uint32), np.empty(ns.value, np.uint32)
        cdf, q = np.empty(pl.value, np.uint32), np.empty(pl.value, np.uint8)
        self._chk(self._lib.tksmseq_get_qscore_model(self._ctx, None, None, None, keys.ctypes.data, off.ctypes.data,
                                                     cnt.ctypes.data, cdf.ctypes.data, q.ctypes.data))
        return {"n_slots": ns.value, "kmer_size": ks.value, "keys": keys, "row_off": off, "row_cnt": cnt,
                "cdf_pool": cdf, "q_pool": q}

    def identity_tables(self):
        c, v, a, b = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self._lib.tksmseq_get_identity(self._ctx, C.byref(c), C.byref(v), C.byref(a), C.byref(b), None))
        qtab = None
        if not c.value:
            qtab = np.empty(65537, np.float64)
            self._chk(self._lib.tksmseq_get_identity(self._ctx, None, None, None, None, qtab.ctypes.data))
        return {"constant": bool(c.value), "value": v.value, "beta_a": a.value, "beta_b": b.value, "qtab": qtab}

    # ---- batches
    def batch_from_mdf(self, text):
        b = text.encode() if isinstance(text, str) else bytes(text)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_batch_from_mdf_text(self._ctx, b, len(b), C.byref(h)))
        return Batch(self, h)

    def molecules_from_mdf(self, text):
        """The parser of the MDF -> MDF modules (tksmseq_molecules_from_mdf_text), which run without a FASTA: a contig name the context
        does not know stays what it is (a literal, printed back by to_mdf_text), substitution positions are not checked."""
        b = text.encode() if isinstance(text, str) else bytes(text)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_molecules_from_mdf_text(self._ctx, b, len(b), C.byref(h)))
        return Batch(self, h)

    def batch_from_arrays(self, reads, intervals, mods=None, literals=None, literal_pool=b"", ids=None, id_pool=b""):
        """Binary layout of include/tksmseq.h (numpy arrays)."""
        reads = np.ascontiguousarray(reads, np.uint32).reshape(-1, 2)
        intervals = np.ascontiguousarray(intervals, np.uint32).reshape(-1, 4)
        mods = np.ascontiguousarray(mods if mods is not None else np.zeros((0, 2)), np.uint32).reshape(-1, 2)
        literals = np.ascontiguousarray(literals if literals is not None else np.zeros((0, 2)), np.uint64).reshape(-1, 2)
        if ids is None:
            ids = np.zeros((len(reads), 2), np.uint32)
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1, 2)
        lp = np.frombuffer(bytes(literal_pool), np.uint8) if not isinstance(literal_pool, np.ndarray) else literal_pool
        ip = np.frombuffer(bytes(id_pool), np.uint8) if not isinstance(id_pool, np.ndarray) else id_pool
        lp, ip = np.ascontiguousarray(lp, np.uint8), np.ascontiguousarray(ip, np.uint8)
        d = L.BatchDesc(len(reads), len(intervals), len(mods), len(literals), len(lp), len(ip), reads.ctypes.data,
                        intervals.ctypes.data, mods.ctypes.data, literals.ctypes.data, lp.ctypes.data, ids.ctypes.data,
                        ip.ctypes.data)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_batch_create(self._ctx, C.byref(d), C.byref(h)))
        return Batch(self, h)

    # ---- molecule-description transforms upstream of Seq (device to device)
    def pcr(self, batch, cycles, target_count, error_rate=None, efficiency=None, preset=None, seed=42, templates=None):
        """PCR::perform (src/pcr.cpp:66-89) on the device; preset: one of the names of src/pcr.cpp:136-140; templates = (begin,
        end): the copies of that slice of the input molecules only (slices, one after the other = the whole)."""
        if preset is not None:
            er, ef = C.c_double(), C.c_double()
            if self._lib.tksmseq_pcr_preset(preset.encode(), C.byref(er), C.byref(ef)):
                raise ValueError(f"Preset {preset} not found")
            error_rate = er.value if error_rate is None else error_rate
            efficiency = ef.value if efficiency is None else efficiency
        if error_rate is None or efficiency is None:
            raise ValueError("Error rate is required!" if error_rate is None else "Efficiency is required!")
        tb, te = templates if templates is not None else (0, 0)
        p = L.PcrParams(seed, target_count, cycles, 0, error_rate, efficiency, tb, te)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_pcr(self._ctx, batch._h, C.byref(p), C.byref(h)))
        return Batch(self, h)

    def pcr_template_counts(self, batch, cycles, target_count, error_rate, efficiency, seed=42):
        """written copies per input molecule (tksmseq_pcr_template_counts)"""
        import numpy as np
        p = L.PcrParams(seed, target_count, cycles, 0, error_rate, efficiency, 0, 0)
        out = np.zeros(batch.n_reads, np.uint64)
        self._chk(self._lib.tksmseq_pcr_template_counts(self._ctx, batch._h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def truncate(self, batch, normal=None, lognormal=None, kde_model=None, always_end=False, kde_models_length=False, seed=42,
                 first_molecule_index=0):
        """truncate_transformer / truncate_transformer_kde (src/truncate.cpp:322-351) on the device: exactly one of normal=(mu,
        sigma), lognormal=(mu, sigma), kde_model=path."""
        if (normal is not None) + (lognormal is not None) + (kde_model is not None) != 1:
            raise ValueError("One of kde-model, normal or lognormal is required!" if normal is None and lognormal is None and kde_model is None
                             else "Only one of kde-model, normal or lognormal is allowed!")
        mode = L.TRC_NORMAL if normal is not None else L.TRC_LOGNORMAL if lognormal is not None else L.TRC_KDE
        mu, sigma = normal if normal is not None else lognormal if lognormal is not None else (0.0, 0.0)
        path = str(kde_model).encode() if kde_model is not None else None
        p = L.TrcParams(seed, first_molecule_index, mode, 1 if always_end else 0, 1 if kde_models_length else 0, 0, mu, sigma, path)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_truncate(self._ctx, batch._h, C.byref(p), C.byref(h)))
        return Batch(self, h)

    # ---- segment edits of the single-cell route (device to device)
    def polya(self, batch, gamma=None, poisson=None, weibull=None, normal=None, min_length=0, max_length=5000, seed=42,
              first_molecule_index=0, comments=True):
        """add_polyA (src/polyA.cpp:133-148) on the device: exactly one of gamma=(shape, scale), poisson=lam, weibull=(shape, scale),
        normal=(mu, sigma)."""
        given = [(d, v) for d, v in ((L.PLA_GAMMA, gamma), (L.PLA_POISSON, poisson), (L.PLA_WEIBULL, weibull), (L.PLA_NORMAL, normal))
                 if v is not None]
        if len(given) != 1:
            raise ValueError("No distribution specified" if not given else "Multiple distributions specified")
        dist, v = given[0]
        a, b = (float(v), 0.0) if dist == L.PLA_POISSON else (float(v[0]), float(v[1]))
        p = L.PolyaParams(seed, first_molecule_index, dist, 0 if comments else L.MOL_NO_COMMENTS, a, b, min_length, max_length)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_polya(self._ctx, batch._h, C.byref(p), C.byref(h)))
        return Batch(self, h)

    def tag(self, batch, format5="", format3="", seed=42, first_molecule_index=0, comments=True):
        """TAG_module::run (src/tag.cpp:70-113) on the device; a format that starts with a digit is that many N's, as the CLI does."""
        def digits(f):
            if f and f[0].isdigit():
                n = 0
                for ch in f:
                    if not ch.isdigit():
                        break
                    n = 10 * n + int(ch)
                return "N" * n
            return f
        format5, format3 = digits(format5 or ""), digits(format3 or "")
        if not format5 and not format3:
            raise ValueError("At least one of the TAG formats must be provided")
        p = L.TagParams(seed, first_molecule_index, format5.encode(), format3.encode(), 0 if comments else L.MOL_NO_COMMENTS, 0)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_tag(self._ctx, batch._h, C.byref(p), C.byref(h)))
        return Batch(self, h)

    def scb(self, batch, keep_meta_barcodes=False, comments=True):
        """SingleCellBarcoder_module::run (src/scb.cpp:57-80) on the device: the CB barcode appended as a segment."""
        p = L.ScbParams(1 if keep_meta_barcodes else 0, 0 if comments else L.MOL_NO_COMMENTS)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_scb(self._ctx, batch._h, C.byref(p), C.byref(h)))
        return Batch(self, h)

    def flip(self, batch, p, seed=42, first_molecule_index=0, comments=True):
        """StrandMan_module (src/strand_man.cpp:37-46) on the device: each molecule flipped with probability p."""
        q = L.FlipParams(seed, first_molecule_index, float(p), 0 if comments else L.MOL_NO_COMMENTS, 0)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_flip(self._ctx, batch._h, C.byref(q), C.byref(h)))
        return Batch(self, h)

    # ---- unsegment and shuffle: glue and reorder molecules (device to device)
    def glue(self, batch, p, seed=42, first_molecule_index=0, comments=True):
        """The loop of Unsegment_module::run (src/unsegment.cpp:88-105) on the device: every unrolled molecule but the first is glued behind
        its predecessor with probability p; a chain becomes one molecule with the head's id and the joiners' ids under the comment key Cat.
        Unlike the reference the last chain is written, and the copies of a depth > 1 record draw one by one (tksmseq_glue)."""
        q = L.GlueParams(seed, first_molecule_index, float(p), 0 if comments else L.MOL_NO_COMMENTS, 0)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_glue(self._ctx, batch._h, C.byref(q), C.byref(h)))
        return Batch(self, h)

    def shuffle(self, batch, seed=42, buffer_size=0, comments=True):
        """Shuffle_module::shuffle_stream (src/shuffle.cpp:23-44) on the device: the unrolled molecules in a uniformly random order
        (buffer_size 0), or in the order the reference's buffer of buffer_size molecules would give -- which does not bound memory here."""
        q = L.ShuffleParams(seed, buffer_size, 0 if comments else L.MOL_NO_COMMENTS, 0)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_shuffle(self._ctx, batch._h, C.byref(q), C.byref(h)))
        return Batch(self, h)

    # ---- mutate: a variant table applied to every segment (device to device)
    def load_variants(self, path=None, text=None):
        """A table of `CONTIG POS MOD` lines (tksmseq_variants_load) from a file or from text: MOD all digits is a deletion of
        [POS, MOD), one letter an SNV, `.SEQ` / `XSEQ` an insertion of SEQ behind POS (X replaces the base at POS)."""
        if (path is None) == (text is None):
            raise ValueError("exactly one of path and text")
        h = C.c_void_p()
        if path is not None:
            self._chk(self._lib.tksmseq_variants_load(self._ctx, str(path).encode(), None, 0, C.byref(h)))
        else:
            b = text.encode() if isinstance(text, str) else bytes(text)
            self._chk(self._lib.tksmseq_variants_load(self._ctx, None, b, len(b), C.byref(h)))
        return Variants(self._lib, h)

    def mutate(self, batch, variants, comments=True):
        """tksmseq_mutate: the SNVs, insertions and deletions of `variants` applied to every (unrolled) molecule of the batch; a perfect
        read of the result is the same slice of the mutated contigs.  No random numbers."""
        q = L.MutateParams(0 if comments else L.MOL_NO_COMMENTS, 0)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_mutate(self._ctx, batch._h, variants._h, C.byref(q), C.byref(h)))
        return Batch(self, h)

    # ---- filter and merge: split and join batches (device to device)
    def filter(self, batch, conditions, negate=False, want_false=True, comments=True):
        """The loop of Filter_module::run (src/filter.cpp:196-212) on the device: conditions as `tksm filter -c` takes them ("info CB",
        "size >=200", "locus chr1:100-200"; one string or a list: all must hold, inverted by negate).  Returns (true_batch, false_batch);
        false_batch is None with want_false=False (that side is then not made)."""
        conditions = [conditions] if isinstance(conditions, (str, bytes)) else list(conditions)
        raw = [c.encode() if isinstance(c, str) else bytes(c) for c in conditions]
        arr = (L.FilterCond * max(1, len(raw)))()
        for k, t in enumerate(raw):
            arr[k].kind, arr[k].text = L.FLT_TEXT, t
        p = L.FilterParams(arr, len(raw), 1 if negate else 0, 0 if comments else L.MOL_NO_COMMENTS)
        ht, hf = C.c_void_p(), C.c_void_p()
        self._chk(self._lib.tksmseq_filter(self._ctx, batch._h, C.byref(p), C.byref(ht), C.byref(hf) if want_false else None))
        return Batch(self, ht), (Batch(self, hf) if want_false else None)

    def merge(self, batches, comments=True):
        """Mrg (`cat` of MDF files) on the device: the molecules of batches[0], then batches[1], ... in one batch (tksmseq_concat)."""
        batches = list(batches)
        arr = (C.c_void_p * max(1, len(batches)))(*[b._h for b in batches])
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_concat(self._ctx, arr, len(batches), 0 if comments else L.MOL_NO_COMMENTS, C.byref(h)))
        return Batch(self, h)

    def append_noise(self, batch, dist, mu, sigma, *, palindromic=False, error_rate=0.5, alphabet="AGTC", seed=42, first=0, comments=True):
        """NoiseAdder::operator() (src/append_noise.cpp:83-128) on the device: a noise length from dist "normal" | "lognormal" (mu, sigma)
        per molecule; a random literal over `alphabet` behind the molecule, or (palindromic) its last segments again, strands toggled,
        with a substitution per hairpin base at error_rate.  first: index of the batch's first molecule in the whole input."""
        if dist not in L.NOISE_DISTS:
            raise ValueError("Distribution not implemented!")
        p = L.NoiseParams(seed, first, L.NOISE_DISTS[dist], 1 if palindromic else 0, float(mu), float(sigma), float(error_rate),
                          str(alphabet).encode(), 0 if comments else L.MOL_NO_COMMENTS, 0)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_append_noise(self._ctx, batch._h, C.byref(p), C.byref(h)))
        return Batch(self, h)

    # ---- model-truncation: the KDE truncation model built on the device
    def kde_grid(self, xy, px, py, bandwidth):
        """KernelDensity(bandwidth).fit(xy).score_samples on the grid px x py, exp'ed (py/truncate_kde.py:245-287), as the EXACT density
        (tksmseq_kde_grid): float64[len(px)][len(py)], P[i][j] for the point (px[i], py[j])."""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        px = np.ascontiguousarray(px, np.float64).ravel(); py = np.ascontiguousarray(py, np.float64).ravel()
        out = np.empty((len(px), len(py)), np.float64)
        self._chk(self._lib.tksmseq_kde_grid(self._ctx, xy.ctypes.data, len(xy), px.ctypes.data, len(px), py.ctypes.data, len(py), float(bandwidth),
                                             out.ctypes.data))
        return out

    def kde_cv_bandwidth(self, xy, seed=42, cv_samples=100000):
        """CV_KDE_bandwidth (py/truncate_kde.py:223-242) with seeded draws (tksmseq_kde_cv_bandwidth): (bandwidth, mean scores float64[3][10]
        for the bandwidths L.KDE_BANDWIDTHS)."""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        bw, scores = C.c_double(), np.empty((3, 10), np.float64)
        self._chk(self._lib.tksmseq_kde_cv_bandwidth(self._ctx, xy.ctypes.data, len(xy), int(seed), int(cv_samples), C.byref(bw), scores.ctypes.data))
        return bw.value, scores

    def model_truncation(self, paf, out, bandwidth=100.0, grid_start=0, grid_end=10000, grid_step=100, model_lengths=False, end_ratio=-1.0, seed=42,
                         cv_samples=100000):
        """main() of py/truncate_kde.py (:323-352): the PAF's primary alignments -> the JSON model `tksm truncate --kde-model` reads."""
        p = L.KdeModelParams(int(seed), int(cv_samples), float(bandwidth), int(grid_start), int(grid_end), int(grid_step), 1 if model_lengths else 0, 0,
                             float(end_ratio))
        self._chk(self._lib.tksmseq_model_truncation(self._ctx, C.byref(p), str(paf).encode(), str(out).encode()))

    # ---- abundance: transcript expression from a PAF by EM on the device
    def abundance(self, paf, out=None, em_iterations=10, lr_br=None, cb_count=0, cb_lognorm_params=(10.0, 1.0), cb_pattern="NNNNNNNNNNNN", cb_dropout=0.2,
                  cb_txt=None, seed=42, keep_hits=False):
        """main() of py/transcript_abundance.py (:326-389) on the device (tksmseq_abundance): the PAF of reads mapped to the transcriptome ->
        {"names", "cells", "tpm": the rows the writer prints, in its order; "abundance": float64 per transcript (order of first appearance,
        "transcripts") before the split; "surviving_reads"; "device_ms"}; the TSV (gzipped for .gz) is written when `out` is given.
        keep_hits: also "reads" (names), "kept" (bool per read), "surviving" (read index), "read_cells" (cell string per surviving read),
        "hit_offsets", "hit_transcripts", "hit_weights" (the final hits per surviving read, in record order)."""
        mu, sigma = cb_lognorm_params
        p = L.AbundanceParams(int(seed), int(em_iterations), 1 if keep_hits else 0, int(cb_count), float(cb_dropout), float(mu), float(sigma),
                              str(cb_pattern).encode(), str(cb_txt).encode() if cb_txt else None, str(lr_br).encode() if lr_br else None)
        h = C.c_void_p()
        self._chk(self._lib.tksmseq_abundance(self._ctx, C.byref(p), str(paf).encode(), C.byref(h)))
        try:
            lib = self._lib
            n = [C.c_uint64() for _ in range(5)]
            lib.tksmseq_abundance_info(h, *[C.byref(v) for v in n])
            rows, surviving, reads, transcripts, hits = [v.value for v in n]
            names, cells, tpm = [], [], np.empty(rows, np.float64)
            a, b, t = C.c_char_p(), C.c_char_p(), C.c_double()
            for i in range(rows):
                lib.tksmseq_abundance_row(h, i, C.byref(a), C.byref(b), C.byref(t))
                names.append(a.value.decode()); cells.append(b.value.decode()); tpm[i] = t.value
            tn = []
            for i in range(transcripts):
                lib.tksmseq_abundance_transcript(h, i, C.byref(a))
                tn.append(a.value.decode())
            vec = C.c_void_p()
            lib.tksmseq_abundance_vector(h, C.byref(vec))
            ms = C.c_float()
            lib.tksmseq_abundance_device_ms(h, C.byref(ms))

            def arr(ptr, count, dtype):
                return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (count * np.dtype(dtype).itemsize,)).view(dtype).copy() if count else np.empty(0, dtype)
            res = {"names": np.array(names, dtype=object), "cells": np.array(cells, dtype=object), "tpm": tpm, "transcripts": np.array(tn, dtype=object),
                   "abundance": arr(vec, transcripts, np.float64), "surviving_reads": surviving, "device_ms": ms.value}
            if keep_hits:
                ptrs = [C.c_void_p() for _ in range(5)]
                if lib.tksmseq_abundance_hits(h, *[C.byref(q) for q in ptrs]):
                    raise TksmSeqError(L.ESTATE, "the hits were not kept")
                k = C.c_int32()
                rn, kept = [], np.zeros(reads, bool)
                for i in range(reads):
                    lib.tksmseq_abundance_read(h, i, C.byref(a), C.byref(k))
                    rn.append(a.value.decode()); kept[i] = bool(k.value)
                cell_ids = arr(ptrs[1], surviving, np.uint32)
                cn = {}
                for c in set(cell_ids.tolist()):
                    lib.tksmseq_abundance_cell(h, c, C.byref(a))
                    cn[c] = a.value.decode()
                res.update(reads=np.array(rn, dtype=object), kept=kept, surviving=arr(ptrs[0], surviving, np.uint32),
                           read_cells=np.array([cn[c] for c in cell_ids.tolist()], dtype=object),
                           hit_offsets=arr(ptrs[2], surviving + 1 if surviving else 0, np.uint32), hit_transcripts=arr(ptrs[3], hits, np.uint32),
                           hit_weights=arr(ptrs[4], hits, np.float64))
            if out is not None and lib.tksmseq_abundance_write(h, str(out).encode()):
                raise TksmSeqError(L.EIO, f"cannot write {out}")
            return res
        finally:
            self._lib.tksmseq_abundance_free(h)

    # ---- model-sequence: Badread error and q-score models built on the device
    def model_sequence(self, reads, alignment, error_out=None, qscore_out=None, error_k=7, qscore_k=9, max_alignments=0, max_alt=25, max_del=6,
                       min_occur=100, max_output=10000, chunk_events=0):
        """`badread error_model` + `badread qscore_model` on the device (tksmseq_model_sequence, the rules in include/tksmseq.h): `reads` (one
        FASTQ path or a list of them, .gz or plain) aligned to the context's reference in `alignment` (a PAF with cg:Z: tags) -> the files
        load_error_model / load_qscore_model read; either output may be None.  Returns the counters of tksmseq_model_sequence_info as a dict."""
        if not isinstance(reads, (list, tuple)):
            reads = [reads]
        p = L.ModelSequenceParams(int(error_k), int(qscore_k), int(max_alignments), int(max_alt), int(max_del), int(min_occur), int(max_output), int(chunk_events))
        info = L.ModelSequenceInfo()
        self._chk(self._lib.tksmseq_model_sequence(self._ctx, C.byref(p), ",".join(str(r) for r in reads).encode(), str(alignment).encode(),
                                                   str(error_out).encode() if error_out else None, str(qscore_out).encode() if qscore_out else None,
                                                   C.byref(info)))
        out = {n: getattr(info, n) for n, _ in L.ModelSequenceInfo._fields_ if n not in ("stage_ms", "reserved")}
        out["stage_ms"] = list(info.stage_ms)
        return out

    def barcode_match(self, reads, whitelist, matches_out, adapter=None, window=200, max_adapter_errors=5, pad=4, max_errors=2, min_exact=2,
                      revcomp_barcodes=False, segments_out=None, selected_out=None, chunk_reads=0):
        """Long reads to cell barcodes on the device (tksmseq_barcode_match, the rules in include/tksmseq.h): `reads` (one FASTQ path or a list
        of them, .gz or plain) and `whitelist` (one barcode per line) -> `matches_out`, the file `abundance(lr_br=...)` reads; optionally the
        segments and the selected barcodes.  Returns the counters of tksmseq_barcode_match_info as a dict."""
        if not isinstance(reads, (list, tuple)):
            reads = [reads]
        p = L.BarcodeMatchParams(adapter.encode() if adapter else None, int(window), int(max_adapter_errors), int(pad), int(max_errors), int(min_exact),
                                 1 if revcomp_barcodes else 0, 0, int(chunk_reads), str(segments_out).encode() if segments_out else None,
                                 str(selected_out).encode() if selected_out else None)
        info = L.BarcodeMatchInfo()
        self._chk(self._lib.tksmseq_barcode_match(self._ctx, C.byref(p), ",".join(str(r) for r in reads).encode(), str(whitelist).encode(),
                                                  str(matches_out).encode(), C.byref(info)))
        out = {n: getattr(info, n) for n, _ in L.BarcodeMatchInfo._fields_ if n not in ("stage_ms", "reserved")}
        out["stage_ms"] = list(info.stage_ms)
        return out

    def map(self, reads, paf_out, k=15, w=10, max_occ=500, max_gap=5000, bandwidth=500, min_count=3, min_score=40, secondary_ratio=0.8, max_secondary=5,
            chunk_reads=0, align=False, eqx=False, align_band=63, extend=False, ext_band=31, ext_drop=40, ext_max=2000, split=False, split_chains=4,
            split_overlap=30, split_segments=8, targets=None, genome_coords=False):
        """Long reads to the contigs of this context's reference (a cDNA FASTA) by minimizer chains on the device (tksmseq_map, the rules in
        include/tksmseq.h): `reads` (one FASTQ path or a list of them, .gz or plain) -> `paf_out`, the PAF `abundance(paf=...)` and
        `model_truncation` read.  align=True (map -c) aligns the written chains base by base (tksmseq_map_align): the lines gain NM:i: and cg:Z:
        tags, which `model_sequence` reads, with = and X in place of M when eqx, inside a band of align_band.  extend=True (map --extend,
        tksmseq_map_extend) moves both ends of every line outward by a banded X-drop extension (band ext_band, drop ext_drop, at most
        ext_max letters an end): the PAF to hand to `model_truncation`.  split=True (map --split, tksmseq_map_split) chains every group in up
        to split_chains rounds and writes a supplementary tp:A:P line for every further piece of a chimeric or hairpin read, at most
        split_segments tp:A:P lines a read, their read intervals sharing at most split_overlap letters.  Returns the counters of
        tksmseq_map_info as a dict, with align=True also those of tksmseq_align_info under "align", with extend=True those of
        tksmseq_extend_info under "extend", with split=True those of tksmseq_split_info under "split".  targets=self.targets() maps to the
        transcripts spliced from genome + GTF instead of the reference's contigs (tksmseq_map_targets); genome_coords=True then writes the
        lines of projectable targets in genome coordinates (N runs in cg:Z:, a tx:Z: tag) and adds the counters of tksmseq_project_info
        under "project"."""
        if genome_coords and targets is None:
            raise ValueError("genome_coords needs targets=")
        if not align and (eqx or align_band != 63):
            raise ValueError("eqx and align_band need align=True")
        if not extend and (ext_band != 31 or ext_drop != 40 or ext_max != 2000):
            raise ValueError("ext_band, ext_drop and ext_max need extend=True")
        if not split and (split_chains != 4 or split_overlap != 30 or split_segments != 8):
            raise ValueError("split_chains, split_overlap and split_segments need split=True")
        if not isinstance(reads, (list, tuple)):
            reads = [reads]
        p = L.MapParams(int(k), int(w), int(max_occ), int(max_gap), int(bandwidth), int(min_count), int(min_score), 0, float(secondary_ratio), int(max_secondary), 0,
                        int(chunk_reads))
        info = L.MapInfo()
        paths = ",".join(str(r) for r in reads).encode()
        ainfo, xinfo, sinfo, pinfo = L.AlignInfo(), L.ExtendInfo(), L.SplitInfo(), L.ProjectInfo()
        if targets is not None:
            ap, xp = L.AlignParams(int(align_band), 1 if eqx else 0), L.ExtendParams(int(ext_band), int(ext_drop), int(ext_max), 0)
            sp = L.SplitParams(int(split_chains), int(split_overlap), int(split_segments), 0)
            tp = L.MapTargetsParams(1 if genome_coords else 0, 0)
            self._chk(self._lib.tksmseq_map_targets(self._ctx, targets._h, C.byref(tp), C.byref(p), C.byref(ap) if align else None, C.byref(xp) if extend else None,
                                                    C.byref(sp) if split else None, paths, str(paf_out).encode(), C.byref(info), C.byref(ainfo), C.byref(xinfo),
                                                    C.byref(sinfo), C.byref(pinfo)))
        elif split:
            ap, xp = L.AlignParams(int(align_band), 1 if eqx else 0), L.ExtendParams(int(ext_band), int(ext_drop), int(ext_max), 0)
            sp = L.SplitParams(int(split_chains), int(split_overlap), int(split_segments), 0)
            self._chk(self._lib.tksmseq_map_split(self._ctx, C.byref(p), C.byref(ap) if align else None, C.byref(xp) if extend else None, C.byref(sp), paths,
                                                  str(paf_out).encode(), C.byref(info), C.byref(ainfo), C.byref(xinfo), C.byref(sinfo)))
        elif extend:
            ap, xp = L.AlignParams(int(align_band), 1 if eqx else 0), L.ExtendParams(int(ext_band), int(ext_drop), int(ext_max), 0)
            self._chk(self._lib.tksmseq_map_extend(self._ctx, C.byref(p), C.byref(ap) if align else None, C.byref(xp), paths, str(paf_out).encode(), C.byref(info),
                                                   C.byref(ainfo), C.byref(xinfo)))
        elif align:
            ap = L.AlignParams(int(align_band), 1 if eqx else 0)
            self._chk(self._lib.tksmseq_map_align(self._ctx, C.byref(p), C.byref(ap), paths, str(paf_out).encode(), C.byref(info), C.byref(ainfo)))
        else:
            self._chk(self._lib.tksmseq_map(self._ctx, C.byref(p), paths, str(paf_out).encode(), C.byref(info)))
        out = {n: getattr(info, n) for n, _ in L.MapInfo._fields_ if n != "stage_ms"}
        out["stage_ms"] = list(info.stage_ms)
        if align:
            out["align"] = {n: getattr(ainfo, n) for n, _ in L.AlignInfo._fields_ if n != "reserved"}
        if extend:
            out["extend"] = {n: getattr(xinfo, n) for n, _ in L.ExtendInfo._fields_ if n != "reserved"}
        if split:
            out["split"] = {n: getattr(sinfo, n) for n, _ in L.SplitInfo._fields_ if n != "reserved"}
        if targets is not None:
            out["project"] = {n: getattr(pinfo, n) for n, _ in L.ProjectInfo._fields_}
        return out

    def targets(self):
        """The transcripts of the table (add_gtf) spliced from this context's reference (the genome) on the device: a Targets."""
        h, info = C.c_void_p(), L.TargetsInfo()
        self._chk(self._lib.tksmseq_targets_from_transcripts(self._ctx, C.byref(h), C.byref(info)))
        return Targets(self, h, info)

    # ---- random-wgs: whole-genome fragments made on the device
    def wgs(self, dist, a, b=0, base_count=None, depth=None, seed=42, first_candidate=0, n_candidates=1 << 20, state=None):
        """The loop of RWGS_module::run (src/random_wgs.cpp:181-207) for candidates [first_candidate, first_candidate + n_candidates)
        of a run (tksmseq_wgs): dist "normal" | "uniform" | "lognormal" | "exponential" with parameters a, b; base_count, or depth
        (base_count = int(depth * reference length)); state = (molecules, bases) emitted by the calls before this one.  Returns
        (batch, state): state = {"next_candidate", "molecules", "bases", "reached"} -- pass first_candidate=state["next_candidate"],
        state=(state["molecules"], state["bases"]) to the next call until reached."""
        if dist not in L.WGS_DISTS:
            raise ValueError("Invalid fragment length distribution")
        if (base_count is None) == (depth is None):
            raise ValueError("Either base-count or depth is required!" if base_count is None else "base_count and depth exclude each other")
        if base_count is None:
            base_count = int(float(depth) * float(self.reference_info()["total_bases"]))
        mols, bases = state if state is not None else (0, 0)
        p = L.WgsParams(seed, L.WGS_DISTS[dist], 0, float(a), float(b), int(base_count), first_candidate, n_candidates, mols, bases)
        h, pr = C.c_void_p(), L.WgsProgress()
        self._chk(self._lib.tksmseq_wgs(self._ctx, C.byref(p), C.byref(h), C.byref(pr)))
        return Batch(self, h), {"next_candidate": pr.next_candidate, "molecules": pr.molecules, "bases": pr.bases, "reached": bool(pr.reached)}

    # ---- transcribe: GTF + abundance tables to molecules, expanded on the device
    def add_gtf(self, path, skip_non_coding=False):
        """read_gtf_transcripts_deep (src/gtf.h:274-304) into the context's transcript table (tksmseq_transcripts_add_gtf); ids the
        table has stay.  skip_non_coding: what the reference passes --default-depth as (src/transcribe.cpp:136)."""
        self._chk(self._lib.tksmseq_transcripts_add_gtf(self._ctx, str(path).encode(), 1 if skip_non_coding else 0))

    def transcripts_info(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.tksmseq_transcripts_info(self._ctx, C.byref(a), C.byref(b)))
        return {"n_transcripts": a.value, "n_exons": b.value}

    def clear_transcripts(self):
        self._chk(self._lib.tksmseq_transcripts_clear(self._ctx))

    def transcribe_plan(self, abundance, molecule_count, *, seed=42, weight=1.0, first_row_index=0, use_whole_id=False, prefix="M", text=None):
        """The count loop of Splicer_module::run (src/transcribe.cpp:149-190) for one abundance table: `abundance` a path (or None with
        text=: the table itself, str or bytes).  weight: this table's share (one table: 1); first_row_index: the data rows of the
        tables before it.  Returns a TranscribePlan: .batch(first, n) makes molecules on the device, .mdf_text() the reference's file."""
        p = L.TsbParams(int(seed), int(molecule_count), float(weight), int(first_row_index), 1 if use_whole_id else 0, 0, str(prefix).encode())
        h = C.c_void_p()
        if abundance is not None:
            rc = self._lib.tksmseq_transcribe_plan_create(self._ctx, str(abundance).encode(), None, 0, C.byref(p), C.byref(h))
        else:
            raw = text.encode() if isinstance(text, str) else bytes(text)
            rc = self._lib.tksmseq_transcribe_plan_create(self._ctx, None, raw, len(raw), C.byref(p), C.byref(h))
        self._chk(rc)
        return TranscribePlan(self, h)

    def transcribe_device_ms(self):
        """(plan ms, write ms): device time of the last transcribe_plan and of the last TranscribePlan.batch, with set_timing(True)"""
        a, b = C.c_float(), C.c_float()
        self._chk(self._lib.tksmseq_transcribe_device_ms(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def to_mdf_text(self, batch):
        """molecule_descriptor::operator<< of every molecule (src/interval.h:898-905)."""
        t, n = C.c_void_p(), C.c_uint64()
        self._chk(self._lib.tksmseq_batch_to_mdf_text(self._ctx, batch._h, C.byref(t), C.byref(n)))
        try:
            return C.string_at(t, n.value).decode()
        finally:
            self._lib.tksmseq_text_free(t)

    # ---- the hot path
    def run(self, batch, target="badread", fastq=True, compute_qual=True, seed=42, first_read_index=0, stride=1,
            collect_stats=False, perfect_of_badread=False):
        p = L.RunParams(seed, first_read_index, stride, L.MODE_BADREAD if target == "badread" else L.MODE_PERFECT,
                        1 if fastq else 0, 1 if compute_qual else 0, 1 if collect_stats else 0,
                        1 if perfect_of_badread else 0, 0)
        r = L.Result()
        self._chk(self._lib.tksmseq_run(self._ctx, batch._h, C.byref(p), C.byref(r)))
        return RunResult(self, r)

    def mdf_to_seq(self, molecules, target="perfect", **kw):
        """molecules: iterable of (molecule_id, [(chrom, start, end, strand, modifications), ...]) exactly as the
        reference's mdf_generator yields them (depth already unrolled).  Returns the formatted records."""
        lines = []
        for mid, intervals in molecules:
            lines.append(f"+{mid}\t1\t\n")
            for chrom, start, end, strand, mods in intervals:
                lines.append(f"{chrom}\t{start}\t{end}\t{strand}\t{mods}\n")
        b = self.batch_from_mdf("".join(lines))
        try:
            return self.run(b, target=target, **kw).records()
        finally:
            b.free()

    def _gzip_fetch(self, g, with_info):
        out = np.empty(g.bytes, np.uint8)
        self._chk(self._lib.tksmseq_gzip_download_range(self._ctx, out.ctypes.data, 0, g.bytes, 0))
        if not with_info:
            return out.tobytes()
        off = np.empty(g.n_members + 1, np.uint64)
        self._chk(self._lib.tksmseq_gzip_download_offsets(self._ctx, off.ctypes.data))
        return out.tobytes(), off, g.device_ms

    def gzip_device(self, ptr, nbytes, format=L.GZIP_RAW, with_info=False):
        """BGZF members of `nbytes` device bytes at `ptr` (tksmseq_gzip_device); format: "raw" / "fasta" / "fastq" or GZIP_*."""
        fmt = {"raw": L.GZIP_RAW, "fasta": L.GZIP_FASTA, "fastq": L.GZIP_FASTQ}.get(format, format)
        g = L.GzipResult()
        self._chk(self._lib.tksmseq_gzip_device(self._ctx, C.c_void_p(ptr) if ptr else None, nbytes, fmt, C.byref(g)))
        return self._gzip_fetch(g, with_info)

    def set_host_threads(self, n):
        """host threads of the MDF parser and writer (tksmseq_set_host_threads; the CLI's -t)"""
        self._chk(self._lib.tksmseq_set_host_threads(self._ctx, int(n)))

    def set_timing(self, on=True):
        self._chk(self._lib.tksmseq_set_timing(self._ctx, 1 if on else 0))

    def run_diagnostics(self):
        """counts of the last Badread run (tksmseq_run_diagnostics): rounds, reads that took the exact kernel, redo share, fall-backs"""
        out = (C.c_uint32 * 16)()
        self._chk(self._lib.tksmseq_run_diagnostics(self._ctx, out))
        # the positions are those of enum RunDiag (csrc/ctx.h), which run.cpp fills by name
        keys = ("rounds", "exact_kernel_reads", "predicted_stragglers", "jobs_14_row_rounds", "jobs_redone_full_width", "fallbacks",
                "fallback_reasons", "fallbacks_qscore_jobs", "fallbacks_list_pass", "jobs_all_rounds", "band_exits")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def set_output_buffer(self, ptr, capacity):
        self._chk(self._lib.tksmseq_set_output_buffer(self._ctx, C.c_void_p(ptr) if ptr else None, capacity))

    def synchronize(self):
        self._chk(self._lib.tksmseq_synchronize(self._ctx))

    def interleave_records(self, streams, offsets, n_per_rank, dst_ptr, dst_capacity):
        n = len(streams)
        sp = (C.c_void_p * n)(*[C.c_void_p(s) for s in streams])
        op = (C.c_void_p * n)(*[C.c_void_p(o) for o in offsets])
        npr = (C.c_uint64 * n)(*n_per_rank)
        out = C.c_uint64()
        self._chk(self._lib.tksmseq_interleave_records(self._ctx, n, sp, op, npr, C.c_void_p(dst_ptr), dst_capacity,
                                                       C.byref(out)))
        return out.value


def random_wgs_main(argv):
    """`tksm random-wgs ...` (src/tksm.cpp); argv[0] == "random-wgs"."""
    lib = L.load()
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    return lib.tksmseq_random_wgs_main(len(argv), arr)


def transcribe_main(argv):
    """`tksm transcribe ...` (src/tksm.cpp); argv[0] == "transcribe"."""
    lib = L.load()
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    return lib.tksmseq_transcribe_main(len(argv), arr)


def sequence_main(argv):
    """The module entry point: `tksm sequence ...` (src/tksm.cpp:164-166); argv[0] == "sequence"."""
    lib = L.load()
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    return lib.tksmseq_sequence_main(len(argv), arr)


def build_tail_model(mapped, unmapped, lx, ly, begin, trans, bandwidth, path, device=0):
    """KDE_noise_generator.from_data + .save (py/tksm_badread.py:888-901, :933-939): the tail-noise model of `tksm sequence --badread-tail-model`
    from (mapped, unmapped) length pairs -- grid[a][b] = density(mapped = lx[a], unmapped = ly[b]) from Sequencer.kde_grid, ratio = share of
    reads with unmapped > 0, bases AGTC, begin / trans the base chain's start weights and 4 x 4 transition weights -- written to `path` as the
    JSON tksmseq_load_tail_model reads.  The reference indexes the grid's rows by ly when it samples, so its layout holds together only for
    axes of equal length: anything else is refused here."""
    import json
    mapped = np.asarray(mapped, np.float64).ravel(); unmapped = np.asarray(unmapped, np.float64).ravel()
    lx = np.asarray(lx, np.float64).ravel(); ly = np.asarray(ly, np.float64).ravel()
    trans = np.asarray(trans, np.float64); begin = np.asarray(begin, np.float64).ravel()
    if len(mapped) != len(unmapped) or len(mapped) == 0:
        raise ValueError("tail model: mapped and unmapped must be non-empty and of one length")
    if len(lx) != len(ly):
        raise ValueError("tail model: lx and ly must have the same length (the reference's sampler reads grid rows by ly)")
    if trans.shape != (4, 4) or begin.shape != (4,):
        raise ValueError("tail model: begin must hold 4 weights, trans 4 x 4")
    s = Sequencer(device)
    try:
        grid = s.kde_grid(np.stack([mapped, unmapped], axis=1), lx, ly, bandwidth)
    finally:
        s.close()
    dc = {"lx": lx.tolist(), "ly": ly.tolist(), "grid": grid.tolist(), "bases": list("AGTC"), "ratio": float(np.sum(unmapped > 0) / len(unmapped)),
          "trans": trans.tolist(), "begin": begin.tolist()}
    with open(path, "w") as f:
        json.dump(dc, f)
    return dc
