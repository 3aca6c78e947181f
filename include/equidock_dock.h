/*
 * equidock_dock.h -- C ABI of libequidock_dock.so: batched inference post-processing for the MI355X (gfx950).
 *
 * Clash removal of src/inference_rigid.py:207-234 (the arithmetic of eqd_clash_iterations, include/equidock_hip.h) for
 * C docked complexes at once.  Conventions as in equidock_hip.h (device pointers unless stated otherwise, the caller owns
 * every buffer, every call enqueues on `stream` and returns without synchronising unless stated otherwise, 0 = EQD_OK or
 * an EQD_ERR_* code), with this library's own ABI version and last-error string.
 *
 * Layout: the complexes are stored one after another.
 *   lig0 [sum n_lig][3]  docked ligand atoms (after apply_rigid), complex c = rows lig_off[c] .. lig_off[c + 1] - 1
 *   rec  [sum n_rec][3]  receptor atoms, complex c = rows rec_off[c] .. rec_off[c + 1] - 1
 *   lig_off / rec_off [C + 1]  HOST int32, lig_off[0] = rec_off[0] = 0, every complex >= 1 atom on each side
 *   states [C]  EqdClashState (euler, trans, loss, it, done) per complex
 *   n_done      one device int32: how many complexes have finished (the host polls these 4 bytes)
 *
 * Per complex, the stop rule of eqd_clash_iterations exactly: the iteration whose loss evaluates <= loss_stop still
 * steps; eta = 1e-3, 1e-4 below loss 2, 1e-2 after iteration 1500; at it == max_it nothing more is evaluated.  A
 * complex's work decomposition depends only on its own sizes and its partial sums are combined in a fixed order, so its
 * results are bit-identical alone, in any batch, at any position and from run to run.
 */
#ifndef EQUIDOCK_DOCK_H
#define EQUIDOCK_DOCK_H

#include <stddef.h>
#include <stdint.h>

#include "equidock_hip.h"   /* EqdClashState, EQD_OK / EQD_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define EQD_DOCK_API __attribute__((visibility("default")))
#else
#define EQD_DOCK_API
#endif

#define EQD_DOCK_ABI_VERSION 1

EQD_DOCK_API int eqd_dock_abi_version(void);
EQD_DOCK_API const char* eqd_dock_last_error(void);
/* 1 when the library is the x86 host simulator build (tests only), else 0 */
EQD_DOCK_API int eqd_dock_is_simulator(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_clash_workspace_bytes(int n_complex, const int32_t* lig_off, const int32_t* rec_off);

/* Validates the offsets, writes the batch's work-item table into the workspace (a host-to-device copy from `max_it`
 * [C], HOST int32, and the offsets; this call waits for that copy) and zeroes `states` and `n_done`. */
EQD_DOCK_API int eqd_dock_clash_init(int n_complex, const int32_t* lig_off, const int32_t* rec_off, const int32_t* max_it,
                                     EqdClashState* states, int32_t* n_done, void* workspace, size_t ws_bytes,
                                     void* stream);

/* Enqueues n_iter iterations (three launches each, whatever C is; no host synchronisation) on a workspace prepared by
 * eqd_dock_clash_init with the same offsets.  A finished complex's work items return at once. */
EQD_DOCK_API int eqd_dock_clash_iterations(int n_iter, int n_complex, const int32_t* lig_off, const int32_t* rec_off,
                                           const float* lig0, const float* rec, float sigma, float surface_ct,
                                           float loss_stop, EqdClashState* states, int32_t* n_done, void* workspace,
                                           size_t ws_bytes, void* stream);

/*
 * Batched graph construction: compute_dig_kNN_graph (src/utils/protein_utils.py:311-397; the arithmetic of
 * eqd_protein_graph_distances / _select / _edges, include/equidock_hip.h) for P proteins in one device pass.  A
 * protein's outputs are bit-identical to the single-protein entry points, alone, in any batch, at any position and
 * from run to run.
 *
 * Layout: the proteins are stored one after another, R = res_off[P] residues and A atoms in all.
 *   res_off [P + 1]        HOST int32, res_off[0] = 0: protein p = residues res_off[p] .. res_off[p + 1] - 1 (>= 1)
 *   prot_atom_off [P + 1]  HOST int32, prot_atom_off[0] = 0: protein p's atoms (= atom_off at its first residue)
 *   atoms [A][3] fp32, atom_off [R + 1] int32 (global atom rows of every residue)
 *   x, n_i, u_i, v_i [R][3] fp64: aligned locations and frame vectors
 * The three size arguments (P, the two host offset arrays, max_neighbor in 1..64) must be the same in every call on a
 * workspace.  Sequence: workspace_bytes -> init (once) -> select -> the host reads edge_off[P] and no_neighbor ->
 * edges with src / dst / he of edge_off[P] rows.
 */
#define EQD_DOCK_GRAPH_ABI 1
EQD_DOCK_API int eqd_dock_graph_abi(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid or a size does not fit 32-bit offsets
 * (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_graph_workspace_bytes(int n_protein, const int32_t* res_off, const int32_t* prot_atom_off,
                                                   int max_neighbor);

/* Validates the offsets and writes the batch's work-item table into the workspace (a host-to-device copy; this call
 * waits for that copy). */
EQD_DOCK_API int eqd_dock_graph_init(int n_protein, const int32_t* res_off, const int32_t* prot_atom_off,
                                     int max_neighbor, void* workspace, size_t ws_bytes, void* stream);

/* Enqueues centroids, distances, neighbour selection + mu_r_norm and the degree scan (one launch each, whatever P is; no
 * host synchronisation).  prune != 0: residue pairs whose atom centroids are at least cutoff + 1e-6 apart are not
 * evaluated (their mean atom distance cannot be below the cutoff), which changes no output.
 *   deg [R] int32, mu_r_norm [R][5] fp32; edge_off [P + 1] int32: first edge of every protein and the total;
 *   no_neighbor [P] int32: a protein's first residue (local index) without a neighbour under the cutoff, or -1;
 *   n_pruned: one int32, the number of residue pairs i < j this call did not evaluate. */
EQD_DOCK_API int eqd_dock_graph_select(int n_protein, const int32_t* res_off, const int32_t* prot_atom_off,
                                       const float* atoms, const int32_t* atom_off, const double* x, double cutoff,
                                       int max_neighbor, int prune, int32_t* deg, int32_t* edge_off, float* mu_r_norm,
                                       int32_t* no_neighbor, int32_t* n_pruned, void* workspace, size_t ws_bytes,
                                       void* stream);

/* Enqueues the edge phase on a workspace eqd_dock_graph_select has filled: src / dst [E] int32 local to each protein,
 * destination-major in the reference's neighbour order, he [E][27] fp32, all in protein order (E = edge_off[P]). */
EQD_DOCK_API int eqd_dock_graph_edges(int n_protein, const int32_t* res_off, const int32_t* prot_atom_off,
                                      int max_neighbor, const double* x, const double* n_i, const double* u_i,
                                      const double* v_i, int32_t* src, int32_t* dst, float* he, void* workspace,
                                      size_t ws_bytes, void* stream);

/*
 * Batched RMSD meter: Meter_Unbound_Bound.update_rmsd (src/utils/eval.py:12-36) and the CRMSD / IRMSD of
 * src/test_all_methods/eval_pdb_outputset.py:80-100 for C complexes in one device pass.  fp64 arithmetic from the fp32
 * inputs; a complex's row of results is bit-identical alone, in any batch, at any position and from run to run.
 *
 * Layout: the complexes are stored one after another, as above.
 *   lig_pred, lig_true [sum n_l][3] fp32, rec_pred, rec_true [sum n_r][3] fp32 (rec_pred may be NULL: it is rec_true)
 *   lig_off / rec_off [C + 1]  HOST int32, starting at 0, every complex >= 1 row on each side
 *   metrics [C][EQD_DOCK_METER_COLS] fp64:
 *     0 ligand RMSD, 1 receptor RMSD (no alignment), 2 complex RMSD (after Kabsch superposition of all rows),
 *     3 interface RMSD: Kabsch RMSD over the pairs (i, j) with |lig_true_i - rec_true_j| < cutoff, a row once per
 *       partner; NaN without such a pair and when interface == 0,
 *     4 the number of interface pairs, 5 flags (bit 0: the complex set took the reflection branch det(V U^T) < 0,
 *       bit 1: the interface set did), 6 and 7: 0
 * Sequence: workspace_bytes -> init (once per set of offsets) -> eval (any number of times).
 */
#define EQD_DOCK_METER_ABI 1
#define EQD_DOCK_METER_COLS 8
EQD_DOCK_API int eqd_dock_meter_abi(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid or do not fit 32-bit offsets
 * (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_meter_workspace_bytes(int n_complex, const int32_t* lig_off, const int32_t* rec_off);

/* Validates the offsets and writes the batch's work-item table into the workspace (a host-to-device copy; this call
 * waits for that copy). */
EQD_DOCK_API int eqd_dock_meter_init(int n_complex, const int32_t* lig_off, const int32_t* rec_off, void* workspace,
                                     size_t ws_bytes, void* stream);

/* Enqueues the metric pass (five launches, four when interface == 0, whatever C is) on a workspace prepared by
 * eqd_dock_meter_init with the same offsets.  No synchronisation, no allocation, no host-device copy: the call can be
 * captured into a hipGraph.  cutoff must be finite and > 0. */
EQD_DOCK_API int eqd_dock_meter_eval(int n_complex, const int32_t* lig_off, const int32_t* rec_off,
                                     const float* lig_pred, const float* rec_pred, const float* lig_true,
                                     const float* rec_true, double cutoff, int interface, double* metrics,
                                     void* workspace, size_t ws_bytes, void* stream);

/*
 * Batched docking quality: fnat, ligand RMSD after superposing the receptors, backbone RMSD of the interface residues
 * and their summary DockQ (Basu & Wallner 2016), plus the steric clashes of the model, for C complexes in one device pass
 * over EVERY heavy atom.  fp64 arithmetic from the fp32 inputs; a complex's row of results is bit-identical alone, in any
 * batch, at any position and from run to run.
 *
 * Layout: the complexes are stored one after another; the model's rows correspond one to one to the native's.
 *   lig_pred, lig_true [A_l][3] fp32, rec_pred, rec_true [A_r][3] fp32 (rec_pred may be NULL: it is rec_true)
 *   lig_atom_off / rec_atom_off [C + 1]  HOST int32, starting at 0: the atom rows of complex c, >= 1 on each side
 *   lig_res_off / rec_res_off [C + 1]    HOST int32, starting at 0: its residues, 1 <= residues <= atoms on each side
 *   lig_res_first [R_l + 1], rec_res_first [R_r + 1]  int32: the first atom row (global) of every residue; a complex's
 *     residues tile its atom rows in order (the kernels hold every range inside the complex's rows whatever the table
 *     says; the host cannot read it, the caller has to get it right)
 *   lig_backbone [A_l], rec_backbone [A_r]  uint8: non-zero for the atoms named N, CA, C or O
 * Definitions: d = sqrt((dx dx + dy dy) + dz dz) < cutoff.  A contact is a (ligand residue, receptor residue) pair with
 * an atom pair under contact_cutoff; N / M / S count the contacts of the native, of the model, of both.  An interface
 * residue has a NATIVE atom pair under interface_cutoff to the other side.
 *   quality [C][EQD_DOCK_QUALITY_COLS] fp64:
 *     0 DockQ = (fnat + 1 / (1 + (iRMSD / 1.5)^2) + 1 / (1 + (LRMSD / 8.5)^2)) / 3, NaN when a term is
 *     1 fnat = S / N (NaN when N = 0), 2 fnonnat = (M - S) / M (0 when M = 0),
 *     3 iRMSD(bb): Kabsch RMSD of the model onto the native over the backbone rows of the interface residues of both
 *       sides (NaN without such a row),
 *     4 LRMSD(bb): the Kabsch transform of rec_pred onto rec_true over the receptor's backbone rows applied to lig_pred,
 *       RMSD to lig_true over the ligand's backbone rows (NaN without a backbone row on either side),
 *     5 N, 6 M, 7 S, 8 / 9 interface residues of the ligand / receptor, 10 interface backbone rows,
 *     11 atom pairs of the model under clash_cutoff, 12 flags (bit 0: the interface set took the reflection branch
 *     det(V U^T) < 0, bit 1: the receptor set did), 13 (residue pair, pose) tests the bound pruned (each residue pair is
 *     tested once in the native and once in the model; 0 with prune == 0), 14 and 15: 0
 * prune != 0: a residue pair of a pose is not evaluated when (distance of the atom centroids - radius - radius) >=
 * max(cutoffs) + 1e-6 - no atom pair of it can be under a cutoff - which changes no other column.
 * Sequence: workspace_bytes -> init (once per set of offsets) -> eval (any number of times).
 */
#define EQD_DOCK_QUALITY_ABI 1
#define EQD_DOCK_QUALITY_COLS 16
EQD_DOCK_API int eqd_dock_quality_abi(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid or do not fit 32-bit offsets
 * (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_quality_workspace_bytes(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                     const int32_t* lig_res_off, const int32_t* rec_res_off);

/* Validates the offsets and writes the batch's work-item table into the workspace (a host-to-device copy; this call
 * waits for that copy). */
EQD_DOCK_API int eqd_dock_quality_init(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                       const int32_t* lig_res_off, const int32_t* rec_res_off, void* workspace,
                                       size_t ws_bytes, void* stream);

/* Enqueues the quality pass (six launches, whatever C is) on a workspace prepared by eqd_dock_quality_init with the
 * same offsets.  No synchronisation, no allocation, no host-device copy: the call can be captured into a hipGraph.
 * Every cutoff must be finite and > 0. */
EQD_DOCK_API int eqd_dock_quality_eval(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                       const int32_t* lig_res_off, const int32_t* rec_res_off, const float* lig_pred,
                                       const float* rec_pred, const float* lig_true, const float* rec_true,
                                       const int32_t* lig_res_first, const int32_t* rec_res_first,
                                       const uint8_t* lig_backbone, const uint8_t* rec_backbone, double contact_cutoff,
                                       double interface_cutoff, double clash_cutoff, int prune, double* quality,
                                       void* workspace, size_t ws_bytes, void* stream);

/*
 * Batched solvent-accessible surface: Shrake-Rupley over EVERY heavy atom of C complexes in one device pass - the SASA of
 * each partner and of the complex, the buried surface area (BSA) and the atoms and residues whose accessibility drops on
 * binding.  It needs no native structure.  fp64 arithmetic from the fp32 inputs, without contraction, exactly as written
 * below; a complex's results are bit-identical alone, in any batch, at any position and from run to run.
 *
 * Layout: the complexes are stored one after another (offsets and residue tables as for the quality pass above).
 *   lig [A_l][3], rec [A_r][3] fp32 heavy-atom rows; lig_radius [A_l], rec_radius [A_r] fp32 atomic radii (finite, > 0: the
 *     caller's to check, the library cannot read them)
 *   lig_atom_off / rec_atom_off / lig_res_off / rec_res_off [C + 1]  HOST int32, as for eqd_dock_quality_*
 *   lig_res_first [R_l + 1], rec_res_first [R_r + 1]  int32: the first atom row (global) of every residue (the kernels hold
 *     every range inside the complex's rows whatever the table says)
 *   sphere [n_points][3] fp64: unit vectors u_k supplied by the caller, 1 <= n_points <= EQD_DOCK_SASA_MAX_POINTS
 *   probe fp64, finite and > 0
 * Definitions.
 *   Expanded radius  R_i = (double)r_i + probe.
 *   Burial           point k of atom i is q = x_i + R_i * u_k per component (one multiply, then one add).  It is buried by
 *                    atom j != i when s = (dx * dx + dy * dy) + dz * dz < R_j * R_j with d = q - x_j.
 *   Counts           every atom has two counts of exposed points: alone (j ranges over the atom's own side) and in complex
 *                    (j ranges over both sides of its complex).  Both come from one walk: same-side partners first, the
 *                    other side only for points still exposed.
 *   Areas            of an atom (4 * pi * R_i * R_i / n_points) * n_i, evaluated left to right; of a residue the sum over
 *                    its atoms in row order; of a side and of the complex the sum over the atoms in row order, ligand
 *                    before receptor; BSA the sum of (4 * pi * R_i * R_i / n_points) * (n_alone_i - n_complex_i) in the
 *                    same order - no cancellation, every term >= 0.
 *   Skipping         a partner is left out of an atom's walk only when it provably buries nothing: the squared centre
 *                    distance (the expression s above on the centres) is >= (R_i + R_j + 1e-6)^2; a whole residue is passed
 *                    over only by a bound on its atoms that implies this for each of them.  The kept partners of an
 *                    atom go on a list of fixed capacity; an atom with more partners than that walks ALL atoms of its
 *                    complex instead, and all_partners != 0 sends every atom down that path.  Both paths give the same
 *                    integers and therefore the same bits, on any input.
 * Outputs.
 *   lig_points [A_l][2], rec_points [A_r][2] int32: exposed points alone, in complex
 *   lig_res_area [R_l][2], rec_res_area [R_r][2] fp64: residue area alone, in complex
 *   rows [C][EQD_DOCK_SASA_COLS] fp64:
 *     0 SASA of the ligand alone, 1 SASA of the receptor alone, 2 SASA of the complex, 3 BSA, 4 / 5 the ligand's / the
 *     receptor's share of the BSA, 6 / 7 buried atoms (n_alone > n_complex) of the ligand / receptor, 8 / 9 buried
 *     residues (>= 1 buried atom) of the ligand / receptor, 10 / 11 exposed points of all atoms alone / in complex
 *     (columns 6-11 are integers stored as fp64)
 * Sequence: workspace_bytes -> init (once per set of offsets) -> eval (any number of times).
 */
#define EQD_DOCK_SASA_ABI 1
#define EQD_DOCK_SASA_COLS 12
#define EQD_DOCK_SASA_MAX_POINTS 1024
EQD_DOCK_API int eqd_dock_sasa_abi(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid, do not fit 32-bit offsets or n_points is outside
 * 1..EQD_DOCK_SASA_MAX_POINTS (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_sasa_workspace_bytes(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                  const int32_t* lig_res_off, const int32_t* rec_res_off, int n_points);

/* Validates the offsets and writes the batch's work-item table into the workspace (a host-to-device copy; this call
 * waits for that copy). */
EQD_DOCK_API int eqd_dock_sasa_init(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                    const int32_t* lig_res_off, const int32_t* rec_res_off, int n_points, void* workspace,
                                    size_t ws_bytes, void* stream);

/* Enqueues the surface pass (five launches, whatever C is) on a workspace prepared by eqd_dock_sasa_init with the same
 * offsets.  No synchronisation, no allocation, no host-device copy: the call can be captured into a hipGraph.  Invalid
 * offsets, n_points outside 1..EQD_DOCK_SASA_MAX_POINTS, a probe that is not finite and > 0 or a workspace that is too
 * small return an EQD_ERR_* code; nothing is launched then. */
EQD_DOCK_API int eqd_dock_sasa_eval(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                    const int32_t* lig_res_off, const int32_t* rec_res_off, const float* lig,
                                    const float* rec, const float* lig_radius, const float* rec_radius,
                                    const int32_t* lig_res_first, const int32_t* rec_res_first, const double* sphere,
                                    int n_points, double probe, int all_partners, int32_t* lig_points, int32_t* rec_points,
                                    double* lig_res_area, double* rec_res_area, double* rows, void* workspace,
                                    size_t ws_bytes, void* stream);

/*
 * Batched residue depth: for EVERY heavy atom of C complexes the distance to the nearest vertex of its protein's surface,
 * alone and in complex, in one device pass - from which the mean and the CA depth of each residue (Chakravarty &
 * Varadarajan 1999; the quantity of the reference's src/surface_analysis.py) and how deep binding buries the interface
 * follow.  The surface is NOT the one of MSMS: a vertex is the van-der-Waals contact point, under the probe, of a
 * Shrake-Rupley sphere point that stays exposed - the contact patch of the solvent-excluded surface.  Re-entrant patches are
 * not modelled, so depths are not comparable digit for digit with Biopython's ResidueDepth; they are defined exactly, below.
 * fp64 arithmetic from the fp32 inputs, without contraction, exactly as written; a complex's results are bit-identical
 * alone, in any batch, at any position and from run to run.
 *
 * Layout and inputs: exactly those of eqd_dock_sasa_* (fp32 rows and radii, HOST int32 atom / residue offsets, device
 * lig_res_first / rec_res_first, the caller's fp64 sphere table u_k with 1 <= n_points <= EQD_DOCK_SASA_MAX_POINTS, an fp64
 * probe, finite and > 0), and
 *   lig_res_ca [R_l], rec_res_ca [R_r]  int32: the global row of each residue's atom named CA (the first such row), or -1
 * Definitions.
 *   Exposure         point k of atom i is exposed alone / in complex by the rule of eqd_dock_sasa_*, unchanged: with
 *                    R_i = (double)r_i + probe and q = x_i + R_i * u_k the point is buried by j != i when
 *                    (dx * dx + dy * dy) + dz * dz < R_j * R_j, d = q - x_j; j ranges over the atom's own side (alone) or
 *                    over both sides (in complex).
 *   Surface vertex   of an exposed point: v_ik = x_i + (double)r_i * u_k per component, one multiply then one add.
 *   Squared depth    s_alone(j): the minimum of (dx * dx + dy * dy) + dz * dz, d = x_j - v_ik, over the alone-exposed vertices
 *                    of j's own side; s_complex(j): the same minimum over the complex-exposed vertices of both sides.  A
 *                    minimum does not depend on the order of its terms.  A side or a complex without any vertex gives
 *                    +inf and sets a flag bit.
 *   Depth            depth = sqrt(s).
 *   Deepened         an atom when s_complex > s_alone (compared on the squared values); a residue when at least one of its
 *                    atoms is.  (depth_complex >= depth_alone is no invariant: the vertices of a clashing partner can lie
 *                    inside an atom's sphere.)
 *   Residue values   mean depth alone / in complex: the sum over the residue's atoms in row order, divided by the count; CA
 *                    depth alone / in complex: the depth of row res_ca, NaN for -1.
 *   Skipping         (prune != 0) a group of vertices - those of a tile of 64 consecutive rows of one side, or those of one
 *                    atom - is passed over for an atom only by a bound that proves none of them beats the atom's running
 *                    minimum: the distance to the group's centre minus the group's reach minus 1e-6, compared against the
 *                    running minimum.  Results are identical with prune on or off on any input; only the count of skipped
 *                    groups differs.
 * Outputs.
 *   lig_depth [A_l][4], rec_depth [A_r][4] fp64: s_alone, s_complex, depth_alone, depth_complex
 *   lig_res_depth [R_l][4], rec_res_depth [R_r][4] fp64: mean alone, mean in complex, CA alone, CA in complex
 *   rows [C][EQD_DOCK_DEPTH_COLS] fp64, all sums in row order, ligand before receptor:
 *     0 / 1 mean atom depth of the ligand / receptor alone, 2 mean atom depth of all atoms in complex, 3 / 4 / 5 the largest
 *     atom depth of the ligand alone / the receptor alone / all atoms in complex, 6 / 7 mean over the ligand's / receptor's
 *     atoms of depth_complex - depth_alone, 8 / 9 deepened atoms of the ligand / receptor, 10 / 11 deepened residues of the
 *     ligand / receptor, 12 / 13 vertices alone / in complex (eqd_dock_sasa_eval's columns 10 / 11 for the same inputs),
 *     14 vertex groups skipped (0 with prune == 0; no other output depends on prune), 15 flags EQD_DOCK_DEPTH_FLAG_*
 *     (columns 8-15 are integers stored as fp64)
 * Sequence: workspace_bytes -> init (once per set of offsets and n_points) -> eval (any number of times).
 */
#define EQD_DOCK_DEPTH_ABI 1
#define EQD_DOCK_DEPTH_COLS 16
#define EQD_DOCK_DEPTH_FLAG_NO_LIGAND_VERTEX 1      /* the ligand alone has no exposed point: its s_alone are +inf */
#define EQD_DOCK_DEPTH_FLAG_NO_RECEPTOR_VERTEX 2    /* the receptor alone has none */
#define EQD_DOCK_DEPTH_FLAG_NO_COMPLEX_VERTEX 4     /* the complex has none: every s_complex is +inf */
EQD_DOCK_API int eqd_dock_depth_abi(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid, do not fit 32-bit offsets or n_points is outside
 * 1..EQD_DOCK_SASA_MAX_POINTS (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_depth_workspace_bytes(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                   const int32_t* lig_res_off, const int32_t* rec_res_off, int n_points);

/* Validates the offsets and writes the batch's tile table into the workspace (a host-to-device copy; this call waits for
 * that copy). */
EQD_DOCK_API int eqd_dock_depth_init(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                     const int32_t* lig_res_off, const int32_t* rec_res_off, int n_points, void* workspace,
                                     size_t ws_bytes, void* stream);

/* Enqueues the depth pass (five launches, whatever C is) on a workspace prepared by eqd_dock_depth_init with the same
 * offsets and n_points.  No synchronisation, no allocation, no host-device copy: the call can be captured into a hipGraph.
 * Invalid offsets, n_points outside 1..EQD_DOCK_SASA_MAX_POINTS, a probe that is not finite and > 0 or a workspace that is
 * too small return an EQD_ERR_* code; nothing is launched then. */
EQD_DOCK_API int eqd_dock_depth_eval(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                     const int32_t* lig_res_off, const int32_t* rec_res_off, const float* lig,
                                     const float* rec, const float* lig_radius, const float* rec_radius,
                                     const int32_t* lig_res_first, const int32_t* rec_res_first, const int32_t* lig_res_ca,
                                     const int32_t* rec_res_ca, const double* sphere, int n_points, double probe, int prune,
                                     double* lig_depth, double* rec_depth, double* lig_res_depth, double* rec_res_depth,
                                     double* rows, void* workspace, size_t ws_bytes, void* stream);

/*
 * Batched lDDT and interface lDDT (Mariani et al. 2013): the superposition-free, atom-level comparison of a model with its
 * native over EVERY heavy atom of C complexes in one device pass - per atom the distances to its native neighbours that
 * the model preserves, from which the lDDT of each residue, of each partner and of the complex follow, and the same
 * restricted to inter-chain pairs (interface lDDT).  fp64 arithmetic from the fp32 inputs, without contraction, exactly as
 * written below; every result is a count of threshold decisions, so a complex's results are bit-identical alone, in any
 * batch, at any position, with prune on or off and from run to run.
 *
 * Layout: that of eqd_dock_quality_*; the complexes are stored one after another and the model's rows correspond one to
 * one to the native's.  The atoms of complex c are its ligand rows followed by its receptor rows.
 *   lig_pred, lig_true [A_l][3] fp32, rec_pred, rec_true [A_r][3] fp32 (rec_pred may be NULL: the model's receptor is rec_true)
 *   lig_atom_off / rec_atom_off / lig_res_off / rec_res_off [C + 1]  HOST int32, as for eqd_dock_quality_*
 *   lig_res_first [R_l + 1], rec_res_first [R_r + 1]  int32: the first atom row (global) of every residue (an atom belongs
 *     to the last residue of its complex and side whose first row is not behind it, whatever else the table says)
 *   inclusion_radius fp64 and thresholds[4] HOST fp64 t_0..t_3, each finite and > 0 (usually 15 and 0.5, 1, 2, 4 Angstrom)
 * Definitions.
 *   Distance         d(i, j) = sqrt((dx * dx + dy * dy) + dz * dz); d_n in the native, d_m in the model.
 *   Included pair    an ordered pair (i, j) of atoms of the same complex that lie in different residues, with
 *                    d_n(i, j) < inclusion_radius.  Two atoms of one entry of a residue table are in the same residue, a
 *                    ligand residue never equals a receptor residue; every unordered pair is counted twice, once for each
 *                    of its atoms.
 *   Preserved        at threshold k when fabs(d_m - d_n) < t_k.
 *   Counts           per atom ten int32: n_all (included partners), p_all[4] (partners preserved per threshold), n_inter,
 *                    p_inter[4] (the same, restricted to partners on the other side).
 *   Score            of any set of atoms (a residue, a side, the complex): (double)(P0 + P1 + P2 + P3) / (4.0 * (double)N)
 *                    with N and P_k the 64-bit integer sums of the atoms' counts; NaN when N == 0.
 *   Pruning          (prune != 0) the rows of each side of a complex are cut into blocks of EQD_DOCK_LDDT_BLOCK consecutive
 *                    rows (the last block of a side may be short).  A block has a native centroid - the row-order fp64 sum
 *                    divided by the count - and a radius, the largest d from the centroid to a row.  An ordered block pair
 *                    (a, b) is not evaluated when (d(centroids) - r_a) - r_b >= inclusion_radius + 1e-6: no atom pair of it
 *                    can be included.  Inside an evaluated block pair the square root is skipped only where
 *                    s >= (inclusion_radius + 1e-6)^2 proves the pair is not included; every decision that counts is made
 *                    with the expressions above.
 * Outputs.
 *   lig_counts [A_l][10], rec_counts [A_r][10] int32: n_all, p_all[4], n_inter, p_inter[4]
 *   lig_res_lddt [R_l][2], rec_res_lddt [R_r][2] fp64: residue lDDT, residue interface lDDT
 *   rows [C][EQD_DOCK_LDDT_COLS] fp64:
 *     0 lDDT (all pairs), 1 interface lDDT (inter-chain pairs only), 2 / 3 lDDT over the ligand's / the receptor's atoms,
 *     4 N (all pairs), 5 N (inter-chain pairs), 6-9 P_k (all pairs), 10-13 P_k (inter-chain pairs), 14 ordered block pairs
 *     skipped by the bound (0 with prune == 0; no other output depends on prune), 15: 0 (columns 4-14 are integers stored
 *     as fp64)
 * Sequence: workspace_bytes -> init (once per set of offsets) -> eval (any number of times).
 */
#define EQD_DOCK_LDDT_ABI 1
#define EQD_DOCK_LDDT_COLS 16
#define EQD_DOCK_LDDT_BLOCK 64
EQD_DOCK_API int eqd_dock_lddt_abi(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid or do not fit 32-bit offsets
 * (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_lddt_workspace_bytes(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                  const int32_t* lig_res_off, const int32_t* rec_res_off);

/* Validates the offsets and writes the batch's work-item table into the workspace (a host-to-device copy; this call
 * waits for that copy). */
EQD_DOCK_API int eqd_dock_lddt_init(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                    const int32_t* lig_res_off, const int32_t* rec_res_off, void* workspace, size_t ws_bytes,
                                    void* stream);

/* Enqueues the lDDT pass (four launches, whatever C is) on a workspace prepared by eqd_dock_lddt_init with the same
 * offsets.  No synchronisation, no allocation, no host-device copy: the call can be captured into a hipGraph.  Invalid
 * offsets, an inclusion_radius or a threshold that is not finite and > 0, or a workspace that is too small return an
 * EQD_ERR_* code; nothing is launched then. */
EQD_DOCK_API int eqd_dock_lddt_eval(int n_complex, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                    const int32_t* lig_res_off, const int32_t* rec_res_off, const float* lig_pred,
                                    const float* rec_pred, const float* lig_true, const float* rec_true,
                                    const int32_t* lig_res_first, const int32_t* rec_res_first, double inclusion_radius,
                                    const double* thresholds, int prune, int32_t* lig_counts, int32_t* rec_counts,
                                    double* lig_res_lddt, double* rec_res_lddt, double* rows, void* workspace,
                                    size_t ws_bytes, void* stream);

/*
 * Batched exact transport plans: the solver call of the pocket OT term, src/utils/ot_utils.py:22-29 (POT's
 * ot.emd(a, b, M) with uniform a = 1/n, b = 1/m), for P problems in ONE launch - the call that replaces the host solver
 * eqd_host_emd_uniform (csrc_host/eqd_host_emd.cpp) and the device <-> host round trip around it.  The algorithm is the
 * host solver's restated operation for operation (successive shortest paths, fp64 from the fp32 costs): a problem's plan
 * is bit-identical to the host solver's, alone, in any batch, at any position and from run to run.
 *
 * Layout (that of eqd_pocket_ot_*): the row blocks of all problems, one after another.
 *   src_off [P + 1]  HOST int32, src_off[0] = 0, non-decreasing: problem p = rows src_off[p] .. src_off[p + 1] - 1 (its n
 *                    sources); a problem of 0 rows is allowed and writes no plan row, as on the host
 *   n_snk            m >= 1 sinks (columns), the same for every problem; n + m <= EQD_DOCK_EMD_MAX_NODES per problem
 *   cost, plan [sum n][n_snk] fp32; every row of a solved plan sums to 1 / n, every column to 1 / m
 *   status [P] int32: 0 solved; 1 the problem failed - no sink with demand could be reached (non-finite costs: the host
 *                    solver returns NaN there) or a loop bound was overrun - and its plan rows are NaN.  Every loop of
 *                    the kernel has a bound computed from n and m: it ends on any input.
 * One workgroup of one wave per problem.  Cost and flow matrices sit in LDS while n * m <=
 * EQD_DOCK_EMD_RESIDENT_CELLS (the resident body), above it the flow sits in the workspace (the general body);
 * `resident` == 0 forces the general body for every problem.  Same operations, same bits.
 * Sequence: workspace_bytes -> init (once per set of offsets) -> solve (any number of times).
 */
#define EQD_DOCK_EMD_ABI 1
#define EQD_DOCK_EMD_MAX_NODES 2048
#define EQD_DOCK_EMD_RESIDENT_CELLS 8192
EQD_DOCK_API int eqd_dock_emd_abi(void);

/* Workspace of a batch with these host offsets; 0 when they are invalid (eqd_dock_last_error says why). */
EQD_DOCK_API size_t eqd_dock_emd_workspace_bytes(int n_problems, const int32_t* src_off, int n_snk);

/* Validates the sizes (EQD_ERR_NULL; EQD_ERR_SHAPE for offsets that do not start at 0 or decrease, n_snk < 1 and a problem
 * of more than EQD_DOCK_EMD_MAX_NODES nodes) and writes the offset table into the workspace (a host-to-device copy; this
 * call waits for that copy). */
EQD_DOCK_API int eqd_dock_emd_init(int n_problems, const int32_t* src_off, int n_snk, void* workspace, size_t ws_bytes,
                                   void* stream);

/* Enqueues the solve (one launch of n_problems workgroups) on a workspace prepared by eqd_dock_emd_init with the same
 * offsets.  No synchronisation, no allocation, no host-device copy: the call can be captured into a hipGraph.  The same
 * validation as init; nothing is launched when it fails. */
EQD_DOCK_API int eqd_dock_emd_solve(int n_problems, const int32_t* src_off, int n_snk, const float* cost, float* plan,
                                    int32_t* status, int resident, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
