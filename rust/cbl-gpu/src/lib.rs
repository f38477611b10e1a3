//! cbl-gpu — `CBL<K, T, PREFIX_BITS>` with the reference's method names, argument meaning and panics for the bulk-insert path
//! (`/root/reference/src/cbl.rs:71-79,127-177,219-228,293-339,358-373,433-449`), every body a call into `libcblx`
//! (`include/cblx.h`). The index lives in the HBM of one MI355X; nothing here computes on the host.
//!
//! NOT compiled in the image this repository was built in (no Rust toolchain there): shipped as source for the maintainer
//! who wires the MI355X path into the reference. Differences from the reference type that a caller can see:
//!   * `T` is the reference's `T` (`build.rs:34-41`: the narrowest integer that holds 2K + POS_BITS bits — `u64` up to K = 29,
//!     `u128` from K = 31 on) and is checked by the reference's own assert (`src/cbl.rs:87-91`); k-mers are packed in it, the
//!     word layout behind the ABI follows from K alone.
//!   * `insert_seq` may only enqueue; every observer (`count`, `contains*`, `save_to_file`, `|=`, `iter`) flushes first, so
//!     results are those of the reference after the same calls.
//!   * out of scope, as in SURVEY.md §8f: `remove`, `remove_seq`, `&=`, `-=`, `^=`, `merge` / `intersect` on vectors of sets,
//!     and the Trie node statistics (`buckets_nodes`, `buckets_node_count`).
//!
//! Drop-in use in `examples/cbl.rs`: replace `use cbl::CBL;` by `use cbl_gpu::CBL;` — nothing else. `write_index(&cbl, path)` /
//! `read_index(path)` (`examples/cbl.rs:117-142`) go through this type's `Serialize` / `Deserialize`, which speak the reference's
//! serde data model (`serde_model.rs`), so bincode `DefaultOptions` + varint writes and reads the reference's bytes.
//! `cbl.save_to_file(path)` / `CBL::load_from_file(path)` (`src/cbl.rs:127-160`) do the same inside the library, on the device
//! (9.4 GB in 0.2 s instead of a host walk). `Build`, `Insert`, `Merge`, `Count`, `Query` run unchanged.
use std::collections::BTreeMap;
use std::ffi::{CStr, CString};
use std::marker::PhantomData;
use std::ops::{BitAnd, BitAndAssign, BitOr, BitOrAssign, BitXor, BitXorAssign, Sub, SubAssign};
use std::os::raw::c_int;
use std::path::Path;

use cblx_sys as sys;

mod serde_model;

/// The integer types a k-mer is packed in (`IntKmer::to_int`, `src/kmer.rs:200-202`: 2K bits, first base most significant).
pub trait PackedInt: Copy {
    const BITS: u32;
    fn split(self) -> (u64, u64);
    fn join(lo: u64, hi: u64) -> Self;
}
impl PackedInt for u64 {
    const BITS: u32 = 64;
    #[inline]
    fn split(self) -> (u64, u64) {
        (self, 0)
    }
    #[inline]
    fn join(lo: u64, _hi: u64) -> Self {
        lo
    }
}
impl PackedInt for u128 {
    const BITS: u32 = 128;
    #[inline]
    fn split(self) -> (u64, u64) {
        (self as u64, (self >> 64) as u64)
    }
    #[inline]
    fn join(lo: u64, hi: u64) -> Self {
        ((hi as u128) << 64) | lo as u128
    }
}

/// A k-mer packed into an integer, as the reference's `IntKmer<K, T>` (with the feature `reference-types` the reference's own
/// type converts from / into this one).
#[derive(Debug, Clone, Copy, PartialEq, Eq, PartialOrd, Ord, Hash)]
#[repr(transparent)]
pub struct IntKmer<const K: usize, T: PackedInt>(pub T);

impl<const K: usize, T: PackedInt> IntKmer<K, T> {
    #[inline]
    pub fn from_int(s: T) -> Self {
        Self(s)
    }
    #[inline]
    pub fn to_int(self) -> T {
        self.0
    }
}

#[cfg(feature = "reference-types")]
mod reference_types {
    use super::{IntKmer, PackedInt};
    use cbl::kmer::{Base, IntKmer as RefKmer, Kmer};

    impl<const K: usize, T: PackedInt + Base> From<RefKmer<K, T>> for IntKmer<K, T> {
        fn from(k: RefKmer<K, T>) -> Self {
            IntKmer(k.to_int())
        }
    }
    impl<const K: usize, T: PackedInt + Base> From<IntKmer<K, T>> for RefKmer<K, T> {
        fn from(k: IntKmer<K, T>) -> Self {
            RefKmer::<K, T>::from_int(k.0)
        }
    }
}

/// A set of k-mers resident in the HBM of one MI355X (`CBL<K, T, PREFIX_BITS>`, `src/cbl.rs:40-54`).
pub struct CBL<const K: usize, T: PackedInt, const PREFIX_BITS: usize = 24> {
    ctx: *mut sys::cblx_ctx,
    _t: PhantomData<T>,
}

// The reference type is not Send / Sync either (UniquePtr members, `src/cbl.rs:50-53`); one ctx = one owner thread.

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> CBL<K, T, PREFIX_BITS> {
    /// Number of bits of a k-mer (`src/cbl.rs:16-18`).
    pub const KMER_BITS: usize = 2 * K;
    /// Number of bits of a position inside a k-mer (`src/cbl.rs:20-22`: ilog2 of 2K rounded up to a power of two).
    pub const POS_BITS: usize = (2 * K).next_power_of_two().trailing_zeros() as usize;

    fn last_error(&self) -> String {
        unsafe { CStr::from_ptr(sys::cblx_last_error(self.ctx)) }.to_string_lossy().into_owned()
    }

    /// A non-zero status becomes the panic the reference would raise, with the library's text
    /// (`CBLX_ESHORT` carries "Sequence size (n) is smaller than K (k)", `src/cbl.rs:329-334`).
    #[inline]
    fn check(&self, rc: c_int) {
        if rc != sys::CBLX_OK {
            panic!("{}", self.last_error());
        }
    }

    fn with(canonical: bool) -> Self {
        // the reference's assert, same condition and text (`src/cbl.rs:87-91`): the word — 2K bits + position — must fit `T`,
        // so `CBL::<31, u64>` (68 bits) panics here exactly as it does there
        assert!(
            Self::KMER_BITS + Self::POS_BITS <= T::BITS as usize,
            "Cannot fit a {K}-mer and its length in a {}-bit integer",
            T::BITS
        );
        let p = sys::cblx_params {
            k: K as u32,
            prefix_bits: PREFIX_BITS as u32,
            canonical: canonical as u32,
            device: -1,
            flags: 0,
            reserved: 0,
        };
        let mut ctx = std::ptr::null_mut();
        let rc = unsafe { sys::cblx_create(&p, &mut ctx) };
        if rc != sys::CBLX_OK {
            // PREFIX_BITS / SUFFIX_BITS asserts of `src/wordset/mod.rs:37-41`, or no usable GPU (there is no CPU fallback)
            panic!("{}", unsafe { CStr::from_ptr(sys::cblx_last_global_error()) }.to_string_lossy());
        }
        Self { ctx, _t: PhantomData }
    }

    /// Creates an empty set (`src/cbl.rs:71-74`).
    pub fn new() -> Self {
        Self::with(false)
    }

    /// Creates an empty set of canonical k-mers (`src/cbl.rs:77-79`).
    pub fn new_canonical() -> Self {
        Self::with(true)
    }

    fn cpath<P: AsRef<Path>>(path: P) -> CString {
        CString::new(path.as_ref().to_str().expect("path is not valid UTF-8")).expect("path contains a NUL byte")
    }

    /// Saves the set to a file: bincode `DefaultOptions` + varint, the bytes of the reference (`src/cbl.rs:127-142`).
    pub fn save_to_file<P: AsRef<Path> + Copy>(&self, path: P) {
        let p = Self::cpath(path);
        let rc = unsafe { sys::cblx_save_to_file(self.ctx, p.as_ptr()) };
        if rc != sys::CBLX_OK {
            panic!("Failed to open {}: {}", path.as_ref().to_str().unwrap(), self.last_error());
        }
    }

    /// Loads a set from a file (`src/cbl.rs:145-160`; trailing bytes are rejected). K / PREFIX_BITS are not in the file:
    /// they are this type's parameters, as in the reference. The canonical flag comes from the file.
    pub fn load_from_file<P: AsRef<Path> + Copy>(path: P) -> Self {
        let s = Self::new();
        let p = Self::cpath(path);
        let rc = unsafe { sys::cblx_load_from_file(s.ctx, p.as_ptr()) };
        if rc != sys::CBLX_OK {
            panic!("Failed to load {}: {}", path.as_ref().to_str().unwrap(), s.last_error());
        }
        s
    }

    /// The exact bytes `save_to_file` writes (for callers that hold a writer instead of a path).
    pub fn to_bytes(&self) -> Vec<u8> {
        let mut n = 0u64;
        self.check(unsafe { sys::cblx_serialized_size(self.ctx, &mut n) });
        let mut buf = vec![0u8; n as usize];
        let mut written = 0u64;
        self.check(unsafe { sys::cblx_serialize(self.ctx, buf.as_mut_ptr(), n, &mut written) });
        buf.truncate(written as usize);
        buf
    }

    /// Inverse of `to_bytes` (`Deserialize`, `src/wordset/mod.rs:398-437`).
    pub fn from_bytes(data: &[u8]) -> Self {
        Self::try_from_bytes(data).unwrap_or_else(|e| panic!("{}", e))
    }

    /// `from_bytes` that reports malformed bytes instead of panicking (what `Deserialize` needs).
    pub fn try_from_bytes(data: &[u8]) -> Result<Self, String> {
        let s = Self::new();
        let rc = unsafe { sys::cblx_load(s.ctx, data.as_ptr(), data.len() as u64) };
        if rc != sys::CBLX_OK {
            return Err(s.last_error());
        }
        Ok(s)
    }

    /// Returns `true` if the set stores canonical k-mers (`src/cbl.rs:164-166`).
    #[inline]
    pub fn is_canonical(&self) -> bool {
        let mut c: c_int = 0;
        self.check(unsafe { sys::cblx_is_canonical(self.ctx, &mut c) });
        c != 0
    }

    /// Counts the k-mers of the set (`src/cbl.rs:169-171`).
    pub fn count(&self) -> usize {
        let mut n = 0u64;
        self.check(unsafe { sys::cblx_count(self.ctx, &mut n) });
        n as usize
    }

    /// Returns `true` if there are no k-mers in the set (`src/cbl.rs:175-177`).
    #[inline]
    pub fn is_empty(&self) -> bool {
        let mut e: c_int = 0;
        self.check(unsafe { sys::cblx_is_empty(self.ctx, &mut e) });
        e != 0
    }

    /// Returns `true` if the set contains the k-mer (`src/cbl.rs:219-221`).
    #[inline]
    pub fn contains(&self, kmer: IntKmer<K, T>) -> bool {
        let (lo, hi) = kmer.to_int().split();
        let mut out = 0u8;
        self.check(unsafe { sys::cblx_contains_kmers(self.ctx, &lo, &hi, 1, &mut out) });
        out != 0
    }

    /// The neighbour mask of a k-mer against the set, the set as the node set of a de Bruijn graph (`Kmer::successors` /
    /// `Kmer::predecessors`, `src/kmer.rs:82-90`, each through `contains`): bit `c` = the successor by base `c` is in the set,
    /// bit `4 + c` = the predecessor by base `c`. The k-mer itself need not be in the set.
    #[inline]
    pub fn neighbors(&self, kmer: IntKmer<K, T>) -> u8 {
        let (lo, hi) = kmer.to_int().split();
        let mut mask = 0u8;
        self.check(unsafe { sys::cblx_neighbors_kmers(self.ctx, &lo, &hi, 1, &mut mask) });
        mask
    }

    /// `table[out][in]` = the k-mers of the set with `out` successors and `in` predecessors in the set; the entries add up to
    /// `count()`. Computed on the device over the whole set.
    pub fn degree_table(&self) -> [[u64; 5]; 5] {
        let mut flat = [0u64; 25];
        self.check(unsafe { sys::cblx_degree_table(self.ctx, flat.as_mut_ptr()) });
        let mut table = [[0u64; 5]; 5];
        for (i, v) in flat.iter().enumerate() {
            table[i / 5][i % 5] = *v;
        }
        table
    }

    /// The ordinal of a k-mer in the iteration order (the index at which `iter` yields it), `None` when the set does not
    /// hold it: the inverse of `iter`.
    #[inline]
    pub fn rank(&self, kmer: IntKmer<K, T>) -> Option<u64> {
        let (lo, hi) = kmer.to_int().split();
        let mut rank = u64::MAX;
        self.check(unsafe { sys::cblx_rank_kmers(self.ctx, &lo, &hi, 1, &mut rank) });
        if rank == u64::MAX { None } else { Some(rank) }
    }

    /// `(k-mers, unitigs, circular unitigs)` of the de Bruijn graph whose nodes are the k-mers of a non-canonical set: the
    /// non-branching paths and the cycles that its simple edges make. Computed on the device; only the counts come back.
    pub fn unitig_counts(&self) -> (u64, u64, u64) {
        let (mut n, mut u, mut c) = (0u64, 0u64, 0u64);
        let null32 = std::ptr::null_mut::<u32>();
        self.check(unsafe {
            sys::cblx_unitig_table(self.ctx, null32, null32, 0, null32, null32, std::ptr::null_mut(), 0, &mut n, &mut u, &mut c)
        });
        (n, u, c)
    }

    /// Writes the unitigs as text to `path` (created or truncated), one line each: the `K` letters of the head, then the
    /// last letter of every following k-mer. Returns `(unitigs, bytes)`.
    pub fn unitigs_to_file<P: AsRef<Path>>(&self, path: P) -> (u64, u64) {
        let cpath = Self::cpath(path);
        let (mut u, mut bytes) = (0u64, 0u64);
        self.check(unsafe { sys::cblx_unitigs_to_file(self.ctx, cpath.as_ptr(), 0, &mut u, &mut bytes) });
        (u, bytes)
    }

    /// `(k-mers, unitigs, circular unitigs)` of a canonical set with odd `K`: the bidirected unitigs, the paths and cycles that
    /// the simple edges between oriented k-mers make, one image of each mirror pair. Only the counts come back.
    pub fn biunitig_counts(&self) -> (u64, u64, u64) {
        let (mut n, mut u, mut c) = (0u64, 0u64, 0u64);
        let null32 = std::ptr::null_mut::<u32>();
        let null8 = std::ptr::null_mut::<u8>();
        self.check(unsafe {
            sys::cblx_biunitig_table(self.ctx, null32, null32, null8, 0, null32, null32, null8, 0, &mut n, &mut u, &mut c)
        });
        (n, u, c)
    }

    /// Writes the bidirected unitigs as text to `path` (created or truncated), one line each: the `K` letters the head spells in
    /// its orientation, then the last letter every following member spells in its own. Returns `(unitigs, bytes)`.
    pub fn biunitigs_to_file<P: AsRef<Path>>(&self, path: P) -> (u64, u64) {
        let cpath = Self::cpath(path);
        let (mut u, mut bytes) = (0u64, 0u64);
        self.check(unsafe { sys::cblx_biunitigs_to_file(self.ctx, cpath.as_ptr(), 0, &mut u, &mut bytes) });
        (u, bytes)
    }

    /// `(unitigs, links)` of the compacted de Bruijn graph: the unitigs of `unitig_counts` (a non-canonical set) or
    /// `biunitig_counts` (a canonical one) and the edges between them. Only the counts come back.
    pub fn gfa_counts(&self) -> (u64, u64) {
        let (mut u, mut l) = (0u64, 0u64);
        self.check(unsafe {
            sys::cblx_gfa_links(self.ctx, std::ptr::null_mut::<u64>(), 0, std::ptr::null_mut::<u32>(), std::ptr::null_mut::<u8>(), 0, &mut u, &mut l)
        });
        (u, l)
    }

    /// Writes the compacted graph as GFA 1.0 to `path` (created or truncated): an `S` line per unitig, an `L` line per link with
    /// the overlap `(K - 1)M`, of a mirror pair of links one line. Returns `(unitigs, L lines, bytes)`.
    pub fn gfa_to_file<P: AsRef<Path>>(&self, path: P) -> (u64, u64, u64) {
        let cpath = Self::cpath(path);
        let (mut u, mut l, mut bytes) = (0u64, 0u64, 0u64);
        self.check(unsafe { sys::cblx_gfa_to_file(self.ctx, cpath.as_ptr(), 0, &mut u, &mut l, &mut bytes) });
        (u, l, bytes)
    }

    /// `[tips, k-mers of the tips, isolated unitigs, k-mers of the isolated unitigs]` at `max_kmers`: a tip is a unitig of at most
    /// `max_kmers` k-mers with exactly one end of degree 0, an isolated unitig one with both. Only the counts come back.
    pub fn tip_counts(&self, max_kmers: u64) -> [u64; 4] {
        let (mut u, mut counts) = (0u64, [0u64; 4]);
        self.check(unsafe { sys::cblx_tips_mark(self.ctx, max_kmers, std::ptr::null_mut::<u8>(), 0, &mut u, counts.as_mut_ptr()) });
        counts
    }

    /// Removes the k-mers of the tips (with `isolated` those of the isolated unitigs too) on the device. A round compacts, marks and
    /// removes every marked unitig of that compaction as one batch; `rounds` = 0 repeats until a round finds nothing.
    pub fn clip_tips(&mut self, max_kmers: u64, isolated: bool, rounds: u32) -> sys::cblx_clip_stats {
        let mut stats = sys::cblx_clip_stats::default();
        let flags = if isolated { sys::CBLX_CLIP_ISOLATED } else { 0 };
        self.check(unsafe { sys::cblx_clip_tips(self.ctx, max_kmers, flags, rounds, &mut stats) });
        stats
    }

    /// `[k-mers, unitigs, links, components, k-mers of the largest component, rounds]` of the connected components of the compacted
    /// de Bruijn graph (a unitig and its reverse complement are one node). Only the counts come back.
    pub fn component_counts(&self) -> [u64; 6] {
        let mut counts = [0u64; 6];
        let (n32, n64) = (std::ptr::null_mut::<u32>(), std::ptr::null_mut::<u64>());
        self.check(unsafe { sys::cblx_components(self.ctx, n32, 0, n32, 0, n32, n32, n64, 0, counts.as_mut_ptr()) });
        counts
    }

    /// Removes whole components on the device as one batch: with `largest` every component but the one of most k-mers (`min_kmers`
    /// must be 0), otherwise every component of fewer than `min_kmers` (at least 1) k-mers.
    pub fn components_filter(&mut self, min_kmers: u64, largest: bool) -> sys::cblx_component_stats {
        let mut stats = sys::cblx_component_stats::default();
        let flags = if largest { sys::CBLX_COMPONENTS_LARGEST } else { 0 };
        self.check(unsafe { sys::cblx_components_filter(self.ctx, min_kmers, flags, &mut stats) });
        stats
    }

    /// Removes the weakly supported k-mers on the device as one batch. `d_counts` is the caller's device array of `n_counts` = `count()`
    /// abundances, one `u32` per stored k-mer by ordinal (what `cblx_abundance_seqs*` tallied). Every k-mer counted fewer than `min_count`
    /// (at least 1) times goes, or with `unitigs` every k-mer of every unitig whose mean count is below `min_count`. The array is only read,
    /// and no longer matches the index after a call that removed something.
    ///
    /// # Safety
    /// `d_counts` must be a device allocation of at least `n_counts` `u32` on the index's device.
    pub unsafe fn abundance_filter(&mut self, d_counts: *const u32, n_counts: u64, min_count: u32, unitigs: bool) -> sys::cblx_abundance_stats {
        let mut stats = sys::cblx_abundance_stats::default();
        let flags = if unitigs { sys::CBLX_ABUNDANCE_UNITIGS } else { 0 };
        self.check(sys::cblx_abundance_filter(self.ctx, d_counts, n_counts, min_count, flags, &mut stats));
        stats
    }

    /// Pops the simple bubbles of the compacted graph on the device: where two to four unitigs of at most `max_kmers` k-mers lead from one unitig end
    /// to the same other end, the one of the highest mean coverage stays and the others are removed, every popped arm of a compaction as one batch;
    /// `rounds` = 0 repeats until a round pops nothing. `d_counts` is the caller's device array of `n_counts` = `count()` abundances (what
    /// `cblx_abundance_seqs*` tallied), carried in place through every removal: afterwards its first `kmers_left` elements are the counts of the
    /// survivors by their new ordinals and the rest is 0. A null `d_counts` with `n_counts` = 0 keeps the longest arm instead.
    ///
    /// # Safety
    /// `d_counts` must be null or a device allocation of at least `n_counts` `u32` on the index's device.
    pub unsafe fn pop_bubbles(&mut self, max_kmers: u64, d_counts: *mut u32, n_counts: u64, rounds: u32) -> sys::cblx_bubble_stats {
        let mut stats = sys::cblx_bubble_stats::default();
        self.check(sys::cblx_pop_bubbles(self.ctx, max_kmers, d_counts, n_counts, 0, rounds, &mut stats));
        stats
    }

    /// Adds a k-mer; returns `true` if it was absent (`src/cbl.rs:226-228`). One device round trip per call: a caller with
    /// many k-mers uses `insert_kmers`.
    #[inline]
    pub fn insert(&mut self, kmer: IntKmer<K, T>) -> bool {
        let (lo, hi) = kmer.to_int().split();
        let mut absent = 0u8;
        self.check(unsafe { sys::cblx_insert_kmers(self.ctx, &lo, &hi, 1, &mut absent) });
        absent != 0
    }

    /// `kmers.iter().map(|k| self.insert(*k)).collect()` in one call.
    pub fn insert_kmers(&mut self, kmers: &[IntKmer<K, T>]) -> Vec<bool> {
        let (lo, hi): (Vec<u64>, Vec<u64>) = kmers.iter().map(|k| k.to_int().split()).unzip();
        let mut absent = vec![0u8; kmers.len()];
        self.check(unsafe { sys::cblx_insert_kmers(self.ctx, lo.as_ptr(), hi.as_ptr(), kmers.len() as u64, absent.as_mut_ptr()) });
        absent.into_iter().map(|b| b != 0).collect()
    }

    /// Removes a k-mer; returns `true` if it was present (`src/cbl.rs:233-235`). One device round trip per call.
    #[inline]
    pub fn remove(&mut self, kmer: IntKmer<K, T>) -> bool {
        let (lo, hi) = kmer.to_int().split();
        let mut present = 0u8;
        self.check(unsafe { sys::cblx_remove_kmers(self.ctx, &lo, &hi, 1, &mut present) });
        present != 0
    }

    fn assert_len(seq: &[u8]) {
        // the reference's assert, before anything is handed over (`src/cbl.rs:294-299,312-317,329-334`)
        assert!(seq.len() >= K, "Sequence size ({}) is smaller than K ({})", seq.len(), K);
    }

    /// Returns `true` if the set contains all the k-mers of a sequence (`src/cbl.rs:293-307`).
    #[inline]
    pub fn contains_all(&mut self, seq: &[u8]) -> bool {
        Self::assert_len(seq);
        let mut out: c_int = 0;
        self.check(unsafe { sys::cblx_contains_all(self.ctx, seq.as_ptr(), seq.len() as u64, &mut out) });
        out != 0
    }

    /// For each k-mer of a sequence, `true` if it is in the set (`src/cbl.rs:311-324`): chunk by chunk, forward-strand words
    /// before reverse-strand ones inside a chunk of a canonical index, as `get_seq_words` orders them.
    #[inline]
    pub fn contains_seq(&mut self, seq: &[u8]) -> Vec<bool> {
        Self::assert_len(seq);
        let cap = (seq.len() - K + 1) as u64;
        let mut out = vec![0u8; cap as usize];
        let mut n = 0u64;
        self.check(unsafe { sys::cblx_contains_seq(self.ctx, seq.as_ptr(), seq.len() as u64, out.as_mut_ptr(), cap, &mut n) });
        out.truncate(n as usize);
        out.into_iter().map(|b| b != 0).collect()
    }

    /// Adds all the k-mers of a sequence (`src/cbl.rs:328-339`). Enqueues; the kernels run at the next observer or `flush`.
    #[inline]
    pub fn insert_seq(&mut self, seq: &[u8]) {
        Self::assert_len(seq);
        self.check(unsafe { sys::cblx_insert_seq(self.ctx, seq.as_ptr(), seq.len() as u64) });
    }

    /// Removes all the k-mers of a sequence (`src/cbl.rs:343-354`). Runs before it returns: pending inserts are applied first.
    #[inline]
    pub fn remove_seq(&mut self, seq: &[u8]) {
        Self::assert_len(seq);
        self.check(unsafe { sys::cblx_remove_seq(self.ctx, seq.as_ptr(), seq.len() as u64) });
    }

    /// The reader loop `for record in reader { cbl.insert_seq(record.seq()) }` (`examples/cbl.rs:154-163`) inside the
    /// library: FASTA / FASTQ, plain or gzip, records in file order. Returns the number of records.
    pub fn insert_fastx_file<P: AsRef<Path> + Copy>(&mut self, path: P) -> u64 {
        let p = Self::cpath(path);
        let mut n = 0u64;
        self.check(unsafe { sys::cblx_insert_fastx_file(self.ctx, p.as_ptr(), &mut n) });
        n
    }

    /// Materialises everything enqueued so far (idempotent; every observer does it first).
    pub fn flush(&mut self) {
        self.check(unsafe { sys::cblx_flush(self.ctx) });
    }

    /// Iterates over the k-mers of the set in the reference's order (`src/cbl.rs:358-361`): prefixes ascending, a Vec bucket in
    /// stored order, a Trie bucket ascending; every word through `revert_necklace_pos`. The k-mers are exported in one call.
    pub fn iter(&self) -> impl Iterator<Item = IntKmer<K, T>> + '_ {
        let n = self.count();
        let (mut lo, mut hi) = (vec![0u64; n], vec![0u64; n]);
        let mut got = 0u64;
        self.check(unsafe { sys::cblx_export_kmers(self.ctx, lo.as_mut_ptr(), hi.as_mut_ptr(), n as u64, &mut got) });
        lo.truncate(got as usize);
        hi.truncate(got as usize);
        lo.into_iter().zip(hi).map(|(l, h)| IntKmer::from_int(T::join(l, h)))
    }

    fn bucket_table(&self) -> (Vec<u32>, Vec<u32>) {
        let mut nb = 0u64;
        self.check(unsafe { sys::cblx_num_buckets(self.ctx, &mut nb) });
        let (mut prefix, mut len) = (vec![0u32; nb as usize], vec![0u32; nb as usize]);
        let mut got = 0u64;
        self.check(unsafe { sys::cblx_bucket_sizes(self.ctx, prefix.as_mut_ptr(), len.as_mut_ptr(), std::ptr::null_mut(), nb, &mut got) });
        prefix.truncate(got as usize);
        len.truncate(got as usize);
        (prefix, len)
    }

    /// Proportion of the available prefixes in use (`src/cbl.rs:364-367`).
    #[inline]
    pub fn prefix_load(&self) -> f64 {
        let mut nb = 0u64;
        self.check(unsafe { sys::cblx_num_buckets(self.ctx, &mut nb) });
        nb as f64 / (1u64 << PREFIX_BITS) as f64
    }

    /// The prefixes of the set with the sizes of their buckets (`src/cbl.rs:370-373`).
    #[inline]
    pub fn buckets_sizes(&self) -> impl Iterator<Item = (usize, usize)> + '_ {
        let (prefix, len) = self.bucket_table();
        prefix.into_iter().zip(len).map(|(p, l)| (p as usize, l as usize))
    }

    /// Number of buckets of each size (`src/cbl.rs:376-379`).
    pub fn buckets_size_count(&self) -> BTreeMap<usize, usize> {
        let mut m = BTreeMap::new();
        for (_, size) in self.buckets_sizes() {
            *m.entry(size).or_insert(0usize) += 1;
        }
        m
    }

    /// Proportion of the k-mers held by the buckets of each size (`src/cbl.rs:382-385`).
    pub fn buckets_load_repartition(&self) -> BTreeMap<usize, f64> {
        let total = self.count() as f64;
        self.buckets_size_count().into_iter().map(|(size, n)| (size, (size * n) as f64 / total)).collect()
    }

    /// The prefixes of the set with the node counts of their buckets (`src/cbl.rs:386-390`): a Vec bucket counts its words, a Trie
    /// bucket its nodes (`TrieVec::count_nodes`), computed on the device.
    pub fn buckets_nodes(&self) -> impl Iterator<Item = (usize, usize)> + '_ {
        let (prefix, _) = self.bucket_table();
        let mut nodes = vec![0u64; prefix.len()];
        let mut got = 0u64;
        self.check(unsafe { sys::cblx_bucket_nodes(self.ctx, nodes.as_mut_ptr(), nodes.len() as u64, &mut got) });
        nodes.truncate(got as usize);
        prefix.into_iter().zip(nodes).map(|(p, n)| (p as usize, n as usize))
    }

    /// Number of buckets for each node count (`src/cbl.rs:392-396`).
    pub fn buckets_node_count(&self) -> BTreeMap<usize, usize> {
        let mut m = BTreeMap::new();
        for (_, nodes) in self.buckets_nodes() {
            *m.entry(nodes).or_insert(0usize) += 1;
        }
        m
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> Default for CBL<K, T, PREFIX_BITS> {
    fn default() -> Self {
        Self::new()
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> Clone for CBL<K, T, PREFIX_BITS> {
    /// `#[derive(Clone)]` of the reference (`src/cbl.rs:40`): `|=` into an empty set clones every bucket as stored (kind and
    /// order kept, `src/wordset/set_ops.rs:123-157`), on the device.
    fn clone(&self) -> Self {
        let s = Self::with(self.is_canonical());
        s.check(unsafe { sys::cblx_merge_assign(s.ctx, self.ctx) });
        s
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> BitOrAssign<&mut Self> for CBL<K, T, PREFIX_BITS> {
    /// Union of `self` and `other` in place (`src/cbl.rs:433-449`). As in the reference, `other`'s Vec buckets that also exist in
    /// `self` end up sorted (`iter_sorted`, `src/trievec/mod.rs:209-220`).
    fn bitor_assign(&mut self, other: &mut Self) {
        assert_eq!(self.is_canonical(), other.is_canonical(), "One of the index is canonical while the other isn't");
        self.check(unsafe { sys::cblx_merge_assign(self.ctx, other.ctx) });
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> CBL<K, T, PREFIX_BITS> {
    /// `let mut c = self.clone(); c |= other; c` without the clone's copy (no reference counterpart as a method: the device merge writes a new
    /// arena anyway, `cblx_merge_from`). `self` is untouched; `other` is left as `|=` leaves it (its Vec buckets that meet a bucket of `self` sorted).
    pub fn merged_with(&self, other: &mut Self) -> Self {
        assert_eq!(self.is_canonical(), other.is_canonical(), "One of the index is canonical while the other isn't");
        let s = Self::with(self.is_canonical());
        s.check(unsafe { sys::cblx_merge_from(s.ctx, self.ctx, other.ctx) });
        s
    }

    /// `(&mut a & &mut b).count()` without the result and without `iter_sorted`'s side effect (no reference counterpart as a method,
    /// `cblx_intersection_count`): the number of k-mers both sets hold; neither set is changed, not even the order inside its Vec buckets.
    pub fn intersection_count(&self, other: &Self) -> usize {
        assert_eq!(self.is_canonical(), other.is_canonical(), "One of the index is canonical while the other isn't");
        let mut n = 0u64;
        self.check(unsafe { sys::cblx_intersection_count(self.ctx, other.ctx, &mut n, std::ptr::null_mut()) });
        n as usize
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> CBL<K, T, PREFIX_BITS> {
    /// `&mut a OP &mut b` (`src/cbl.rs:411-431, 451-471, 491-511, 531-551`): a new set; both operands keep theirs, with their Vec buckets on the
    /// prefixes both hold sorted (`iter_sorted`).
    fn set_op(&mut self, other: &mut Self, op: u32) -> Self {
        assert_eq!(self.is_canonical(), other.is_canonical(), "One of the index is canonical while the other isn't");
        let s = Self::with(self.is_canonical());
        s.check(unsafe { sys::cblx_set_op(s.ctx, self.ctx, other.ctx, op) });
        s
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> CBL<K, T, PREFIX_BITS> {
    fn set_op_many(cbls: Vec<&mut Self>, op: u32) -> Self {
        assert!(!cbls.is_empty() && cbls.len() <= sys::CBLX_SETOP_MAX_OPERANDS as usize);
        let canonical = cbls[0].is_canonical();
        assert!(cbls.iter().all(|c| c.is_canonical() == canonical), "One of the index is canonical while the other isn't");
        let s = Self::with(canonical);
        let srcs: Vec<*mut sys::cblx_ctx> = cbls.iter().map(|c| c.ctx).collect();
        s.check(unsafe { sys::cblx_set_op_many(s.ctx, srcs.as_ptr(), srcs.len() as u32, op) });
        s
    }

    /// Union of many sets (`src/cbl.rs:106-114`): a bucket one operand holds is cloned as stored, a bucket several hold becomes an ascending Vec and the
    /// Vec buckets of those holders end up sorted (`iter_sorted`).
    pub fn merge(cbls: Vec<&mut Self>) -> Self {
        Self::set_op_many(cbls, sys::CBLX_SETOP_OR)
    }

    /// Intersection of many sets (`src/cbl.rs:116-124`): only prefixes all operands hold are visited.
    pub fn intersect(cbls: Vec<&mut Self>) -> Self {
        Self::set_op_many(cbls, sys::CBLX_SETOP_AND)
    }

    /// `contains_seq` of every sequence against every set of a panel in one pass (no reference counterpart, `cblx_contains_seqs_counts_many`): sequence `i` is
    /// `bases[offsets[i]..offsets[i + 1]]`. Returns `(total, positive)`: `total[i]` k-mers of sequence `i` were queried and `positive[j][i]` of them are
    /// in `cbls[j]`. The k-mers are encoded and partitioned once for the whole panel; no set is changed, not even the order inside its Vec buckets.
    pub fn contains_seqs_counts_many(cbls: Vec<&mut Self>, bases: &[u8], offsets: &[u64]) -> (Vec<u32>, Vec<Vec<u32>>) {
        assert!(!cbls.is_empty() && cbls.len() <= sys::CBLX_SETOP_MAX_OPERANDS as usize);
        let canonical = cbls[0].is_canonical();
        assert!(cbls.iter().all(|c| c.is_canonical() == canonical), "One of the index is canonical while the other isn't");
        let nseq = offsets.len().saturating_sub(1);
        for w in offsets.windows(2) {
            assert!(w[1] >= w[0] && (w[1] - w[0]) as usize >= K, "Sequence size ({}) is smaller than K ({})", w[1].saturating_sub(w[0]), K);
        }
        assert!(offsets.last().map_or(true, |&e| e as usize <= bases.len()));
        let srcs: Vec<*mut sys::cblx_ctx> = cbls.iter().map(|c| c.ctx).collect();
        let mut total = vec![0u32; nseq];
        let mut rows = vec![0u32; srcs.len() * nseq];
        cbls[0].check(unsafe {
            sys::cblx_contains_seqs_counts_many(
                srcs.as_ptr(),
                srcs.len() as u32,
                bases.as_ptr(),
                offsets.as_ptr(),
                nseq as u64,
                total.as_mut_ptr(),
                rows.as_mut_ptr(),
                std::ptr::null_mut(),
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
            )
        });
        let positive = if nseq == 0 { vec![Vec::new(); srcs.len()] } else { rows.chunks(nseq).map(|r| r.to_vec()).collect() };
        (total, positive)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> BitAnd<Self> for &mut CBL<K, T, PREFIX_BITS> {
    type Output = CBL<K, T, PREFIX_BITS>;
    /// Intersection (`src/cbl.rs:451-471`).
    fn bitand(self, other: Self) -> Self::Output {
        self.set_op(other, sys::CBLX_SETOP_AND)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> Sub<Self> for &mut CBL<K, T, PREFIX_BITS> {
    type Output = CBL<K, T, PREFIX_BITS>;
    /// Difference (`src/cbl.rs:491-511`).
    fn sub(self, other: Self) -> Self::Output {
        self.set_op(other, sys::CBLX_SETOP_SUB)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> BitXor<Self> for &mut CBL<K, T, PREFIX_BITS> {
    type Output = CBL<K, T, PREFIX_BITS>;
    /// Symmetric difference (`src/cbl.rs:531-551`).
    fn bitxor(self, other: Self) -> Self::Output {
        self.set_op(other, sys::CBLX_SETOP_XOR)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> CBL<K, T, PREFIX_BITS> {
    /// `a OP= &mut b` (`src/cbl.rs:473-489, 513-529, 553-569`): in place, with the reference's bucket layout; `other` keeps its set, with its Vec
    /// buckets on the prefixes both hold sorted (`iter_sorted`).
    fn set_op_assign(&mut self, other: &mut Self, op: u32) {
        assert_eq!(self.is_canonical(), other.is_canonical(), "One of the index is canonical while the other isn't");
        self.check(unsafe { sys::cblx_set_op_assign(self.ctx, other.ctx, op) });
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> BitAndAssign<&mut Self> for CBL<K, T, PREFIX_BITS> {
    /// Intersection in place (`src/cbl.rs:473-489`).
    fn bitand_assign(&mut self, other: &mut Self) {
        self.set_op_assign(other, sys::CBLX_SETOP_AND)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> SubAssign<&mut Self> for CBL<K, T, PREFIX_BITS> {
    /// Difference in place (`src/cbl.rs:513-529`).
    fn sub_assign(&mut self, other: &mut Self) {
        self.set_op_assign(other, sys::CBLX_SETOP_SUB)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> BitXorAssign<&mut Self> for CBL<K, T, PREFIX_BITS> {
    /// Symmetric difference in place (`src/cbl.rs:553-569`).
    fn bitxor_assign(&mut self, other: &mut Self) {
        self.set_op_assign(other, sys::CBLX_SETOP_XOR)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> BitOr<Self> for &mut CBL<K, T, PREFIX_BITS> {
    type Output = CBL<K, T, PREFIX_BITS>;
    /// Union into a new set (`src/cbl.rs:411-431`); `|=` is the in-place form.
    fn bitor(self, other: Self) -> Self::Output {
        self.set_op(other, sys::CBLX_SETOP_OR)
    }
}

impl<const K: usize, T: PackedInt, const PREFIX_BITS: usize> Drop for CBL<K, T, PREFIX_BITS> {
    fn drop(&mut self) {
        unsafe { sys::cblx_destroy(self.ctx) }
    }
}

#[cfg(test)]
mod tests {
    //! The reference's own membership tests for this surface (`src/cbl.rs:591-773`), restated; they need an MI355X.
    use super::*;

    const K: usize = 31;
    type T = u128; // 2K + POS_BITS = 68 bits (`build.rs:34-41`)

    fn seq(n: usize, seed: u64) -> Vec<u8> {
        let mut x = seed;
        (0..n)
            .map(|_| {
                x = x.wrapping_add(0x9E3779B97F4A7C15);
                let mut z = x;
                z = (z ^ (z >> 30)).wrapping_mul(0xBF58476D1CE4E5B9);
                z = (z ^ (z >> 27)).wrapping_mul(0x94D049BB133111EB);
                b"ACGT"[((z ^ (z >> 31)) & 3) as usize]
            })
            .collect()
    }

    #[test]
    fn insert_seq_then_contains_all() {
        let s = seq(10_000, 42);
        let mut cbl = CBL::<K, T>::new();
        cbl.insert_seq(&s);
        assert!(cbl.contains_all(&s));
        assert_eq!(cbl.contains_seq(&s).len(), s.len() - K + 1);
        assert!(cbl.count() <= s.len() - K + 1);
    }

    #[test]
    fn union_and_round_trip() {
        let (a, b) = (seq(5_000, 1), seq(5_000, 2));
        let (mut x, mut y) = (CBL::<K, T>::new(), CBL::<K, T>::new());
        x.insert_seq(&a);
        y.insert_seq(&b);
        x |= &mut y;
        assert!(x.contains_all(&a) && x.contains_all(&b));
        let z = CBL::<K, T>::from_bytes(&x.to_bytes());
        assert_eq!(z.count(), x.count());
        assert_eq!(z.to_bytes(), x.to_bytes());
    }

    /// `write_index` / `read_index` of `examples/cbl.rs:117-142` through this type's serde impls: the bytes bincode writes are the
    /// bytes `save_to_file` writes, and they read back to the same index (needs the dev-dependency `bincode = "1.3"`).
    #[test]
    fn serde_model_is_the_file_format() {
        use bincode::{DefaultOptions, Options};
        let mut cbl = CBL::<K, T>::new();
        for seed in 0..40 {
            cbl.insert_seq(&seq(3_000, seed)); // enough words under one prefix for both kinds of bucket
        }
        let opts = || DefaultOptions::new().with_varint_encoding().reject_trailing_bytes();
        let via_serde = opts().serialize(&cbl).unwrap();
        assert_eq!(via_serde, cbl.to_bytes());
        let back: CBL<K, T> = opts().deserialize(&via_serde).unwrap();
        assert_eq!(back.count(), cbl.count());
        assert_eq!(back.to_bytes(), via_serde);
    }

    #[test]
    #[should_panic(expected = "Cannot fit a 31-mer and its length in a 64-bit integer")]
    fn word_must_fit_the_integer_type() {
        let _ = CBL::<31, u64>::new(); // `src/cbl.rs:87-91`
    }

    #[test]
    #[should_panic(expected = "is smaller than K")]
    fn short_sequence_panics() {
        CBL::<K, T>::new().insert_seq(b"ACGT");
    }
}
