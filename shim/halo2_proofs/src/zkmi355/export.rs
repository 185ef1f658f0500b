//! `ConstraintSystem` + keygen `Assembly`  ->  key blob v4 (layout: INTEGRATION.md §3; parsed by
//! `zk_pk_create`, csrc/prover.hip).  The Python mirror of this file is
//! `zkevm-circuits_amd/plonk.py::Circuit::{cs_blob, blob}`, which the tests use.
//!
//! Everything the verifier can see is taken from upstream's own data, never re-derived:
//!   * query order      = `cs.advice_queries` / `fixed_queries` / `instance_queries` (registration order:
//!                        the order of the evaluations in the proof)
//!   * lookup arguments = `cs.lookups` AFTER `chunk_lookups()` [REF zkevm-circuits/src/super_circuit/test.rs:59]:
//!                        one table tuple + N input tuples each (mv-lookup)
//!   * degree           = `cs.degree()`, blinding factors = `cs.blinding_factors()`
//!   * selectors        already compressed into fixed columns by `compress_selectors` (keygen does it
//!                        before the blob is written), so `Expression::Selector` cannot occur
use ff::PrimeField;
use halo2curves::bn256::Fr;

use crate::plonk::{Any, Column, ConstraintSystem, Expression};
use crate::poly::Rotation;

// opcodes of the library's postfix evaluator (csrc/quotient.hip)
const Q_PUSH_COL: u32 = 1;
const Q_PUSH_CONST: u32 = 2;
const Q_ADD: u32 = 3;
const Q_SUB: u32 = 4;
const Q_MUL: u32 = 5;
const Q_NEG: u32 = 6;
const Q_MUL_CONST: u32 = 10;
const CT_FIXED: u32 = 0;
const CT_ADVICE: u32 = 1;
const CT_INSTANCE: u32 = 2;
const C_CHAL0: u32 = 0xFFFD_0000; // C_CHAL0 + i = halo2 `Challenge` i
const BLOB_MAGIC: u32 = 0x4B50_5A4B;
const BLOB_VERSION: u32 = 4; // typed fixed cells + `Assembly::mapping`: the device builds the sigma columns

pub(super) struct Blob {
    pub bytes: Vec<u8>,
    consts: Vec<Fr>,
}

fn put_u32(out: &mut Vec<u8>, v: u32) {
    out.extend_from_slice(&v.to_le_bytes());
}
/// `Fr` as it lives in memory: 4 x u64 Montgomery limbs (== SerdeFormat::RawBytes).
fn put_fr(out: &mut Vec<u8>, v: &Fr) {
    // SAFETY: halo2curves' Fr is #[repr(transparent)] over [u64; 4] (Montgomery form)
    let limbs: &[u64; 4] = unsafe { &*(v as *const Fr as *const [u64; 4]) };
    for l in limbs {
        out.extend_from_slice(&l.to_le_bytes());
    }
}
pub(super) fn fr_slice_bytes(col: &[Fr]) -> &[u8] {
    // SAFETY: see put_fr; a column crosses the ABI as its in-memory form
    unsafe { std::slice::from_raw_parts(col.as_ptr() as *const u8, col.len() * 32) }
}

impl Blob {
    fn constant(&mut self, v: Fr) -> u32 {
        if let Some(i) = self.consts.iter().position(|c| *c == v) {
            return i as u32;
        }
        self.consts.push(v);
        (self.consts.len() - 1) as u32
    }

    /// halo2 `Expression` -> postfix program (op, a, b) triples.
    fn compile(&mut self, e: &Expression<Fr>, prog: &mut Vec<[u32; 3]>) {
        match e {
            Expression::Constant(c) => {
                let i = self.constant(*c);
                prog.push([Q_PUSH_CONST, i, 0]);
            }
            Expression::Selector(_) => panic!("selectors must be compressed into fixed columns before the export (keygen does)"),
            Expression::Fixed(q) => prog.push([Q_PUSH_COL, (CT_FIXED << 24) | q.column_index() as u32, q.rotation().0 as u32]),
            Expression::Advice(q) => prog.push([Q_PUSH_COL, (CT_ADVICE << 24) | q.column_index() as u32, q.rotation().0 as u32]),
            Expression::Instance(q) => prog.push([Q_PUSH_COL, (CT_INSTANCE << 24) | q.column_index() as u32, q.rotation().0 as u32]),
            Expression::Challenge(c) => prog.push([Q_PUSH_CONST, C_CHAL0 + c.index() as u32, 0]),
            Expression::Negated(a) => {
                self.compile(a, prog);
                prog.push([Q_NEG, 0, 0]);
            }
            Expression::Sum(a, b) => {
                // a + (-b) is how halo2 writes a subtraction: emit SUB directly
                if let Expression::Negated(nb) = &**b {
                    self.compile(a, prog);
                    self.compile(nb, prog);
                    prog.push([Q_SUB, 0, 0]);
                } else {
                    self.compile(a, prog);
                    self.compile(b, prog);
                    prog.push([Q_ADD, 0, 0]);
                }
            }
            Expression::Product(a, b) => {
                self.compile(a, prog);
                self.compile(b, prog);
                prog.push([Q_MUL, 0, 0]);
            }
            Expression::Scaled(a, f) => {
                self.compile(a, prog);
                let i = self.constant(*f);
                prog.push([Q_MUL_CONST, i, 0]);
            }
        }
    }
}

fn put_prog(out: &mut Vec<u8>, prog: &[[u32; 3]]) {
    put_u32(out, prog.len() as u32);
    for ins in prog {
        for w in ins {
            put_u32(out, *w);
        }
    }
}
fn put_queries<C>(out: &mut Vec<u8>, queries: &[(Column<C>, Rotation)])
where
    C: crate::plonk::ColumnType,
{
    put_u32(out, queries.len() as u32);
    for (col, rot) in queries {
        put_u32(out, col.index() as u32);
        put_u32(out, rot.0 as u32);
    }
}

/// Narrowest cell width of a version 4 fixed column: 1, 2, 4, 8 or 16 bytes of little-endian unsigned integer when every
/// cell's canonical value fits, else 32 (the column then goes as it lives in memory, Montgomery form).
fn cell_width(col: &[Fr]) -> usize {
    let mut used = 1;
    for v in col {
        let repr = v.to_repr(); // canonical, little-endian
        let bytes = repr.as_ref();
        let top = bytes.iter().rposition(|b| *b != 0).map_or(0, |i| i + 1);
        used = used.max(top);
    }
    [1usize, 2, 4, 8, 16].into_iter().find(|w| used <= *w).unwrap_or(32)
}

/// `fixed` = the fixed columns after selector compression (n values each), `mapping` = `permutation::keygen::Assembly::mapping`
/// as keygen left it: mapping[j][i] = (j', i'), the next cell in the cycle of cell i of permutation column j.
pub(super) fn key_blob(cs: &ConstraintSystem<Fr>, k: u32, fixed: &[Vec<Fr>], mapping: &[Vec<(usize, usize)>]) -> Vec<u8> {
    let mut b = Blob { bytes: Vec::new(), consts: Vec::new() };
    // programs first (they fill the constant pool), serialised after the header
    let gates: Vec<Vec<[u32; 3]>> = cs
        .gates()
        .iter()
        .flat_map(|g| g.polynomials().iter())
        .map(|poly| {
            let mut p = Vec::new();
            b.compile(poly, &mut p);
            p
        })
        .collect();
    let lookups: Vec<(Vec<Vec<[u32; 3]>>, Vec<Vec<Vec<[u32; 3]>>>)> = cs
        .lookups()
        .iter()
        .map(|arg| {
            let table = arg
                .table_expressions()
                .iter()
                .map(|e| {
                    let mut p = Vec::new();
                    b.compile(e, &mut p);
                    p
                })
                .collect();
            let inputs = arg
                .input_expressions()
                .iter()
                .map(|tuple| {
                    tuple
                        .iter()
                        .map(|e| {
                            let mut p = Vec::new();
                            b.compile(e, &mut p);
                            p
                        })
                        .collect()
                })
                .collect();
            (table, inputs)
        })
        .collect();
    let perm: Vec<Column<Any>> = cs.permutation().get_columns();
    let phases = cs.advice_column_phase(); // Vec<u8>, one per advice column
    let chal = cs.challenge_phase(); // Vec<u8>, one per challenge
    let out = &mut b.bytes;
    for v in [
        BLOB_MAGIC,
        BLOB_VERSION,
        k,
        cs.blinding_factors() as u32,
        cs.degree() as u32,
        cs.num_fixed_columns() as u32,
        cs.num_advice_columns() as u32,
        cs.num_instance_columns() as u32,
        perm.len() as u32,
        lookups.len() as u32,
        gates.len() as u32,
        b.consts.len() as u32,
    ] {
        put_u32(out, v);
    }
    put_u32(out, chal.len() as u32);
    for p in &phases {
        put_u32(out, *p as u32);
    }
    for p in &chal {
        put_u32(out, *p as u32);
    }
    put_queries(out, cs.advice_queries());
    put_queries(out, cs.fixed_queries());
    put_queries(out, cs.instance_queries());
    for col in &perm {
        let t = match col.column_type() {
            Any::Fixed => CT_FIXED,
            Any::Advice(_) => CT_ADVICE,
            Any::Instance => CT_INSTANCE,
        };
        put_u32(out, t);
        put_u32(out, col.index() as u32);
    }
    for c in &b.consts {
        put_fr(out, c);
    }
    for g in &gates {
        put_prog(out, g);
    }
    for (table, inputs) in &lookups {
        put_u32(out, table.len() as u32);
        put_u32(out, inputs.len() as u32);
        for p in table {
            put_prog(out, p);
        }
        for tuple in inputs {
            for p in tuple {
                put_prog(out, p);
            }
        }
    }
    assert_eq!(fixed.len(), cs.num_fixed_columns());
    assert_eq!(mapping.len(), perm.len());
    let widths: Vec<usize> = fixed.iter().map(|col| cell_width(col)).collect();
    for w in &widths {
        put_u32(out, *w as u32);
    }
    for (col, w) in fixed.iter().zip(&widths) {
        assert_eq!(col.len(), 1usize << k);
        if *w == 32 {
            out.extend_from_slice(fr_slice_bytes(col));
        } else {
            for v in col {
                out.extend_from_slice(&v.to_repr().as_ref()[..*w]);
            }
        }
    }
    for col in mapping {
        assert_eq!(col.len(), 1usize << k);
        for (j, i) in col {
            put_u32(out, *j as u32);
            put_u32(out, *i as u32);
        }
    }
    let _ = <Fr as PrimeField>::NUM_BITS;
    std::mem::take(&mut b.bytes)
}
