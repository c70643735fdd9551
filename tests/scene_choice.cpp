/* TEST INFRASTRUCTURE - the scene gq_step_call.h model_scene picks for a GqModelDesc, next to what the model's own self-collision pair table
 * holds (tests/test_scene_choice.py).  Built by tests/scene_split_build.py with the host emulator's flags; no product export is involved. */
#include "gq_device.h"          /* the emulator shim (tests/simt_emu comes first on the include path) */
#include "gq_step_call.h"
#include "emu_model.h"

/* out[0] the scene; out[1] self pairs, out[2] those of kind 1 - 3 (exact box routines), out[3] those of kind 4 (convex routine), out[4] the
 * model's ncvx_self; out[5 .. 8] scene_boxes / scene_self / scene_prim / scene_cvx of the scene.  0, or -1 with the text in err. */
extern "C" int scene_choice(const GqModelDesc* desc, int32_t* out, char* err, int errlen) {
  static EmuModel m;
  if (emu_build_model(desc, m, err, errlen)) return -1;
  const GqDevModel& M = m.M;
  int box = 0, cvx = 0;
  for (int p = 0; p < M.nsp; p++) { const int k = M.sp[p].kind; box += k >= 1 && k <= 3; cvx += k == 4; }
  const gq::Scene s = gq::model_scene(M);
  out[0] = s; out[1] = M.nsp; out[2] = box; out[3] = cvx; out[4] = M.ncvx_self;
  out[5] = gq::scene_boxes(s); out[6] = gq::scene_self(s); out[7] = gq::scene_prim(s); out[8] = gq::scene_cvx(s);
  return 0;
}
