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

#ifdef __cplusplus
}
#endif

#endif
