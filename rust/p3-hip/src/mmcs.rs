//! `Mmcs<Val>` on the GPU: the `ValMmcs` / `ChallengeMmcs` aliases of
//! `bin/src/config.rs:19-20` (`MerkleTreeMmcs<Val, Val, Hash, Compress, 1>`).
//! Same commitment and proof types as MerkleTreeMmcs (`Hash<Val, Val, 1>`,
//! `Vec<[Val; 1]>`), so proofs and verifiers are interchangeable.  The tree
//! layers stay in HBM (`lsp_tree`); the committed matrices stay on the host
//! because `TwoAdicFriPcs` reads them back through `get_matrices`.
use std::sync::Arc;

use p3_commit::Mmcs;
use p3_field::FieldAlgebra;
use p3_matrix::{Dimensions, Matrix};
use p3_symmetric::Hash;

use crate::{fr1, fr_ptr, fr_ptr_mut, sys, Ctx, Val};

#[derive(Clone)]
pub struct HipMmcs {
    ctx: Arc<Ctx>,
}

impl HipMmcs {
    pub fn new(ctx: Arc<Ctx>) -> Self {
        HipMmcs { ctx }
    }
}

impl Default for HipMmcs {
    fn default() -> Self {
        HipMmcs { ctx: crate::global() }
    }
}

/// `ProverData<M>`: the device tree plus the committed host matrices
pub struct HipTree<M> {
    tree: *mut sys::lsp_tree,
    leaves: Vec<M>,
    height: usize, // of the tallest matrices
    widths: Vec<usize>,
}

// lsp_tree is only read after commit, under the owning context's mutex
unsafe impl<M: Send> Send for HipTree<M> {}
unsafe impl<M: Sync> Sync for HipTree<M> {}

impl<M> Drop for HipTree<M> {
    fn drop(&mut self) {
        unsafe { sys::lsp_tree_free(self.tree) };
    }
}

#[derive(Debug)]
pub enum HipMmcsError {
    WrongBatchSize,
    WrongWidth,
    /// heights are powers of two, the library-wide rule (p3 pads others)
    HeightNotPowerOfTwo,
    IndexOutOfRange,
    /// a batch of several heights beyond lsp_merkle_commit_mixed's limits
    UnsupportedBatch,
    WrongProofLength,
    RootMismatch,
}

impl Mmcs<Val> for HipMmcs {
    type ProverData<M> = HipTree<M>;
    type Commitment = Hash<Val, Val, 1>;
    type Proof = Vec<[Val; 1]>;
    type Error = HipMmcsError;

    /// lsp_merkle_commit_mixed: the tallest matrices make the leaves (leaf i =
    /// hash_iter(row i of each, in order)); the matrices of every smaller
    /// height are hashed row by row and injected at the level with as many
    /// nodes, node = compress(compress(left, right), hash_iter(rows)) -- p3's
    /// MerkleTree::new.  Heights are powers of two (the library-wide rule).
    /// Matrices of one height -- every commit of this prover: trace, quotient
    /// chunks, one FRI round -- go to lsp_merkle_commit, which computes the
    /// same tree byte for byte and finishes its top on the host.
    fn commit<M: Matrix<Val>>(&self, inputs: Vec<M>) -> (Self::Commitment, Self::ProverData<M>) {
        assert!(!inputs.is_empty(), "HipMmcs::commit of no matrices");
        // any M: Matrix -> one contiguous host copy per matrix for the upload
        // (host memory holds the matrices twice while this runs)
        let staged: Vec<Vec<Val>> = inputs.iter().map(|m| m.rows().flatten().collect()).collect();
        let ptrs: Vec<*const sys::lsp_fr> = staged.iter().map(|v| fr_ptr(v)).collect();
        let widths: Vec<usize> = inputs.iter().map(|m| m.width()).collect();
        let heights: Vec<usize> = inputs.iter().map(|m| m.height()).collect();
        let height = *heights.iter().max().unwrap();
        let mut root = [Val::ZERO];
        let mut tree: *mut sys::lsp_tree = std::ptr::null_mut();
        if heights.iter().all(|&h| h == height) {
            let rc = unsafe {
                sys::lsp_merkle_commit(
                    self.ctx.raw(),
                    ptrs.as_ptr(),
                    widths.as_ptr(),
                    ptrs.len(),
                    height,
                    sys::LSP_MEM_HOST,
                    fr_ptr_mut(&mut root),
                    &mut tree,
                )
            };
            self.ctx.check(rc, "lsp_merkle_commit");
        } else {
            let rc = unsafe {
                sys::lsp_merkle_commit_mixed(
                    self.ctx.raw(),
                    ptrs.as_ptr(),
                    widths.as_ptr(),
                    heights.as_ptr(),
                    ptrs.len(),
                    sys::LSP_MEM_HOST,
                    fr_ptr_mut(&mut root),
                    &mut tree,
                )
            };
            self.ctx.check(rc, "lsp_merkle_commit_mixed");
        }
        (Hash::from(root), HipTree { tree, leaves: inputs, height, widths })
    }

    /// Row `index >> log2(height / h_j)` of every matrix, in commit order, and
    /// the log2(height) siblings; `index` counts the tallest matrices' rows.
    fn open_batch<M: Matrix<Val>>(&self, index: usize, d: &HipTree<M>) -> (Vec<Vec<Val>>, Self::Proof) {
        let mut rows = vec![Val::ZERO; d.widths.iter().sum()];
        let mut path = vec![Val::ZERO; d.height.trailing_zeros() as usize];
        let rc = unsafe { sys::lsp_merkle_open(d.tree, index, fr_ptr_mut(&mut rows), fr_ptr_mut(&mut path)) };
        self.ctx.check(rc, "lsp_merkle_open");
        let mut opened = Vec::with_capacity(d.widths.len());
        let mut off = 0;
        for &w in &d.widths {
            opened.push(rows[off..off + w].to_vec());
            off += w;
        }
        (opened, path.into_iter().map(|x| [x]).collect())
    }

    fn get_matrices<'a, M: Matrix<Val>>(&self, d: &'a HipTree<M>) -> Vec<&'a M> {
        d.leaves.iter().collect()
    }

    /// lsp_merkle_verify (one height) or lsp_merkle_verify_mixed on the host
    /// (the verifier never needs a GPU): `dimensions` in commit order, as
    /// p3's MerkleTreeMmcs takes them
    fn verify_batch(
        &self,
        commit: &Self::Commitment,
        dimensions: &[Dimensions],
        index: usize,
        opened_values: &[Vec<Val>],
        proof: &Self::Proof,
    ) -> Result<(), Self::Error> {
        if dimensions.is_empty() || dimensions.len() != opened_values.len() {
            return Err(HipMmcsError::WrongBatchSize);
        }
        if dimensions.iter().zip(opened_values).any(|(d, r)| d.width != r.len()) {
            return Err(HipMmcsError::WrongWidth);
        }
        if dimensions.iter().any(|d| !d.height.is_power_of_two()) {
            return Err(HipMmcsError::HeightNotPowerOfTwo);
        }
        let height = dimensions.iter().map(|d| d.height).max().unwrap();
        let log_height = height.trailing_zeros();
        if proof.len() != log_height as usize {
            return Err(HipMmcsError::WrongProofLength);
        }
        let widths: Vec<usize> = dimensions.iter().map(|d| d.width).collect();
        let rows: Vec<Val> = opened_values.iter().flatten().copied().collect();
        let path: Vec<Val> = proof.iter().map(|d| d[0]).collect();
        let root: [Val; 1] = (*commit).into();
        // one height: lsp_merkle_verify, as before (any number of matrices)
        if dimensions.iter().all(|d| d.height == height) {
            let rc = unsafe {
                sys::lsp_merkle_verify(
                    self.ctx.raw(),
                    fr1(&root[0]),
                    widths.as_ptr(),
                    widths.len(),
                    log_height,
                    index,
                    fr_ptr(&rows),
                    fr_ptr(&path),
                )
            };
            return match rc {
                sys::LSP_OK => Ok(()),
                sys::LSP_E_VERIFY => Err(HipMmcsError::RootMismatch),
                _ => {
                    self.ctx.check(rc, "lsp_merkle_verify");
                    unreachable!()
                }
            };
        }
        if index >= height {
            return Err(HipMmcsError::IndexOutOfRange);
        }
        if widths.iter().any(|&w| w == 0) {
            return Err(HipMmcsError::WrongWidth);
        }
        let heights: Vec<usize> = dimensions.iter().map(|d| d.height).collect();
        let rc = unsafe {
            sys::lsp_merkle_verify_mixed(
                self.ctx.raw(),
                fr1(&root[0]),
                widths.as_ptr(),
                heights.as_ptr(),
                widths.len(),
                index,
                fr_ptr(&rows),
                fr_ptr(&path),
            )
        };
        match rc {
            sys::LSP_OK => Ok(()),
            sys::LSP_E_VERIFY => Err(HipMmcsError::RootMismatch),
            // what lsp_merkle_commit_mixed cannot have committed: more than 8
            // matrices of one height, a width or height beyond its limits
            sys::LSP_E_ARG | sys::LSP_E_SIZE => Err(HipMmcsError::UnsupportedBatch),
            _ => {
                self.ctx.check(rc, "lsp_merkle_verify_mixed");
                unreachable!()
            }
        }
    }
}
