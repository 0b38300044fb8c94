//! Any `Air` as an `LSP_AIR_PROGRAM` config (include/lsp.h): the symbolic
//! constraints p3-uni-stark itself derives (`get_symbolic_constraints`) lowered
//! to the straight-line register program the library's quotient, check and
//! verifier interpret.  Mirrors `linea_stark_prover_amd/air.py`
//! (`ProgramBuilder.build`): equal subexpressions are one node, each
//! expression runs its costlier side first (Sethi-Ullman), a shared node keeps
//! its slot until its last use, and more than 16 live values is an error.
//!
//! ```ignore
//! let desc = p3_hip::program::descriptor(&[p3_hip::program::lower(&air, num_public_values)?]);
//! ```
//! Public values stay `[alpha, delta, ...]` on the library's side only by
//! convention of the built-in configs: a program may read any index.
//! Periodic columns, several trace phases and extension fields are outside the
//! format.  Preprocessed columns have a config type of their own on the
//! library's side (`LSP_AIR_PROGRAM_PREP`, operand kinds 8 `PREP_LOCAL` and 9
//! `PREP_NEXT`; include/lsp.h), which this lowering does not emit: the fork's
//! uni-stark has no preprocessed trace, so such an entry stays `Unsupported`.
use std::collections::HashMap;
use std::rc::Rc;

use p3_air::Air;
use p3_uni_stark::{get_symbolic_constraints, Entry, SymbolicAirBuilder, SymbolicExpression};

use crate::sys::{self, LSP_AIR_PROGRAM};
use crate::Val;

pub const MAX_SLOTS: usize = 16;
const SLOT: i32 = 0;
const LOCAL: i32 = 1;
const NEXT: i32 = 2;
const PUBLIC: i32 = 3;
const CONST: i32 = 4;
const FIRST: i32 = 5;
const LAST: i32 = 6;
const TRANS: i32 = 7;
/// `LSP_AIR_PROGRAM_PREP` only (config type 4: `4, width, prep_width, nslots, ...`):
/// a cell of the preprocessed matrix in the row of `LOCAL` / `NEXT`.  Named here
/// for readers of a descriptor; `lower` emits neither (see the module comment).
pub const PREP_LOCAL: i32 = 8;
pub const PREP_NEXT: i32 = 9;
pub const PROGRAM_PREP_TYPE: i32 = sys::LSP_AIR_PROGRAM_PREP;
const ADD: i32 = 1;
const SUB: i32 = 2;
const MUL: i32 = 3;
const ASSERT_ZERO: i32 = 4;

#[derive(Debug)]
pub enum LowerError {
    /// more than 16 values live at once
    TooManySlots,
    /// a preprocessed / permutation / challenge entry, or a row offset past 1
    Unsupported(&'static str),
    /// past 2^16 constants, 2^20 ops or 2^20 columns
    TooLarge(&'static str),
}

/// One encoded program config (the words after the descriptor's config count).
pub struct Program {
    pub width: usize,
    pub nslots: usize,
    pub words: Vec<i32>,
}

#[derive(Clone, Copy, PartialEq, Eq, Hash)]
enum Node {
    Leaf(i32, u32), // kind, payload (a constant's payload is its index in `consts`)
    Op(i32, usize, usize),
}

struct Graph {
    nodes: Vec<Node>,
    ids: HashMap<Node, usize>,
    consts: Vec<[u32; 8]>,
    const_ids: HashMap<[u32; 8], u32>,
    // the symbolic tree shares subtrees through Rc: one visit per allocation
    seen: HashMap<*const SymbolicExpression<Val>, usize>,
}

fn canonical_words(v: &Val) -> [u32; 8] {
    // Val crosses the ABI as lsp_fr (lib.rs asserts the size): the library
    // turns the Montgomery words into the canonical ones
    let mut c = [0u64; 4];
    unsafe { sys::lsp_fr_to_canonical(v as *const Val as *const sys::lsp_fr, c.as_mut_ptr()) };
    let mut w = [0u32; 8];
    for i in 0..4 {
        w[2 * i] = c[i] as u32;
        w[2 * i + 1] = (c[i] >> 32) as u32;
    }
    w
}

impl Graph {
    fn node(&mut self, n: Node) -> usize {
        if let Some(&i) = self.ids.get(&n) {
            return i;
        }
        self.nodes.push(n);
        self.ids.insert(n, self.nodes.len() - 1);
        self.nodes.len() - 1
    }

    fn constant(&mut self, v: &Val) -> Result<usize, LowerError> {
        let w = canonical_words(v);
        let next = self.consts.len() as u32;
        let i = *self.const_ids.entry(w).or_insert(next);
        if i == next {
            if next >= 1 << 16 {
                return Err(LowerError::TooLarge("more than 2^16 constants"));
            }
            self.consts.push(w);
        }
        Ok(self.node(Node::Leaf(CONST, i)))
    }

    fn add(&mut self, e: &Rc<SymbolicExpression<Val>>) -> Result<usize, LowerError> {
        let key = Rc::as_ptr(e);
        if let Some(&i) = self.seen.get(&key) {
            return Ok(i);
        }
        let i = self.expr(e)?;
        self.seen.insert(key, i);
        Ok(i)
    }

    fn expr(&mut self, e: &SymbolicExpression<Val>) -> Result<usize, LowerError> {
        use SymbolicExpression as E;
        Ok(match e {
            E::Variable(v) => match v.entry {
                Entry::Main { offset: 0 } => self.node(Node::Leaf(LOCAL, v.index as u32)),
                Entry::Main { offset: 1 } => self.node(Node::Leaf(NEXT, v.index as u32)),
                Entry::Public => self.node(Node::Leaf(PUBLIC, v.index as u32)),
                Entry::Main { .. } => return Err(LowerError::Unsupported("row offset past 1")),
                _ => return Err(LowerError::Unsupported("preprocessed, permutation or challenge entry")),
            },
            E::IsFirstRow => self.node(Node::Leaf(FIRST, 0)),
            E::IsLastRow => self.node(Node::Leaf(LAST, 0)),
            E::IsTransition => self.node(Node::Leaf(TRANS, 0)),
            E::Constant(c) => self.constant(c)?,
            E::Add { x, y, .. } => {
                let (a, b) = (self.add(x)?, self.add(y)?);
                self.node(Node::Op(ADD, a, b))
            }
            E::Sub { x, y, .. } => {
                let (a, b) = (self.add(x)?, self.add(y)?);
                self.node(Node::Op(SUB, a, b))
            }
            E::Mul { x, y, .. } => {
                let (a, b) = (self.add(x)?, self.add(y)?);
                self.node(Node::Op(MUL, a, b))
            }
            E::Neg { x, .. } => {
                let (z, a) = (self.constant(&Val::default())?, self.add(x)?);
                self.node(Node::Op(SUB, z, a))
            }
        })
    }
}

/// Lower `air`'s constraints, in the order its `eval` asserts them.
pub fn lower<A>(air: &A, num_public_values: usize) -> Result<Program, LowerError>
where
    A: Air<SymbolicAirBuilder<Val>>,
{
    let width = air.width();
    if width == 0 || width > 1 << 20 {
        return Err(LowerError::TooLarge("width outside [1, 2^20]"));
    }
    let constraints = get_symbolic_constraints(air, 0, num_public_values);
    let mut g = Graph { nodes: vec![], ids: HashMap::new(), consts: vec![], const_ids: HashMap::new(), seen: HashMap::new() };
    let mut roots = Vec::with_capacity(constraints.len());
    for c in &constraints {
        roots.push(g.expr(c)?);
    }
    // uses per node (one per referencing edge and per assert) and the
    // Sethi-Ullman need; a leaf is an operand and needs no slot
    let n = g.nodes.len();
    let mut uses = vec![0u32; n];
    let mut reach = vec![false; n];
    for &r in &roots {
        uses[r] += 1;
        let mut st = vec![r];
        while let Some(i) = st.pop() {
            if let Node::Op(_, a, b) = g.nodes[i] {
                if !reach[i] {
                    reach[i] = true;
                    for c in [a, b] {
                        uses[c] += 1;
                        st.push(c);
                    }
                }
            }
        }
    }
    let mut need = vec![0u32; n];
    for i in 0..n {
        // operands have lower ids than the node that names them
        if let (true, Node::Op(_, a, b)) = (reach[i], g.nodes[i]) {
            let (x, y) = (need[a], need[b]);
            need[i] = 1.max(if x == y { x + 1 } else { x.max(y) });
        }
    }
    let mut ops: Vec<[i32; 4]> = vec![];
    let mut slot_of: HashMap<usize, usize> = HashMap::new();
    let mut free: Vec<usize> = (0..MAX_SLOTS).rev().collect(); // lowest on top
    let mut top = 0usize;
    let operand = |g: &Graph, slot_of: &HashMap<usize, usize>, i: usize| -> i32 {
        match g.nodes[i] {
            Node::Leaf(kind, v) => kind << 24 | v as i32,
            Node::Op(..) => SLOT << 24 | slot_of[&i] as i32,
        }
    };
    fn release(g: &Graph, uses: &mut [u32], slot_of: &mut HashMap<usize, usize>, free: &mut Vec<usize>, i: usize) {
        uses[i] -= 1;
        if let (Node::Op(..), 0) = (g.nodes[i], uses[i]) {
            free.push(slot_of.remove(&i).unwrap());
            free.sort_unstable_by(|a, b| b.cmp(a));
        }
    }
    for &root in &roots {
        let mut st = vec![(root, false)];
        while let Some((i, ready)) = st.pop() {
            let Node::Op(code, a, b) = g.nodes[i] else { continue };
            if slot_of.contains_key(&i) {
                continue;
            }
            if !ready {
                st.push((i, true));
                let (first, second) = if need[a] >= need[b] { (a, b) } else { (b, a) };
                st.push((second, false));
                st.push((first, false));
                continue;
            }
            let (oa, ob) = (operand(&g, &slot_of, a), operand(&g, &slot_of, b));
            release(&g, &mut uses, &mut slot_of, &mut free, a);
            release(&g, &mut uses, &mut slot_of, &mut free, b);
            let s = free.pop().ok_or(LowerError::TooManySlots)?;
            top = top.max(s + 1);
            slot_of.insert(i, s);
            ops.push([code, s as i32, oa, ob]);
        }
        ops.push([ASSERT_ZERO, 0, operand(&g, &slot_of, root), 0]);
        release(&g, &mut uses, &mut slot_of, &mut free, root);
    }
    if ops.len() > 1 << 20 {
        return Err(LowerError::TooLarge("more than 2^20 ops"));
    }
    let mut words = vec![LSP_AIR_PROGRAM, width as i32, top as i32, g.consts.len() as i32, ops.len() as i32,
                         roots.len() as i32];
    for c in &g.consts {
        words.extend(c.iter().map(|&w| w as i32));
    }
    for o in &ops {
        words.extend_from_slice(o);
    }
    Ok(Program { width, nslots: top, words })
}

/// The descriptor of an AIR made of these programs, in order.
pub fn descriptor(programs: &[Program]) -> Vec<i32> {
    let mut d = vec![programs.len() as i32];
    for p in programs {
        d.extend_from_slice(&p.words);
    }
    d
}
