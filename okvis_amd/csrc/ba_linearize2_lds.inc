// Part of ba_linearize2.hpp, included in the body of linearize2_kernel and of linearize2_rec_kernel: where everything lies in the
// workgroup's dynamic LDS (smem), and the work-item's indices.
  constexpr int RECD = Lin2Cfg<REAL, FUSE, UB>::REC_DOUBLES;
  REAL* s_rec = reinterpret_cast<REAL*>(smem);   // [pieces][16] piece records; then [pairs][27] block records in slot order
  double* s_pair = smem;                         // phase A: [pairs][3]
  double* s_lm = smem + RECD;                    // [GROUP_LM][4] trial landmarks
  double* s_lmres = s_lm + GROUP_LM * 4;         // [GROUP_LM][16] landmark sums (V 6, b 3, H_l 6, cost)
  double* s_sc = s_lmres + GROUP_LM * 16;        // [4][64] per-landmark step scalars of phase A
  double* s_pose = s_sc + 4 * 64;                // [LIN2_POSES][7] trial poses of the window
  double* s_cam = s_pose + LIN2_POSES * 7;       // [LIN2_CAMS][12]
  int* s_lpb = reinterpret_cast<int*>(s_cam + LIN2_CAMS * 12);   // [GROUP_LM + 1] first piece of each landmark
  int* s_pp = s_lpb + GROUP_LM + 1;              // [LIN2_PIECES] pair -> first piece | count << 16
  int* s_poff = s_pp + LIN2_PIECES;              // [LIN2_PIECES] reduced offset of the pair's block
  int* s_task = s_poff + LIN2_PIECES;            // [LIN_TASK_CACHE][6]
  int* s_cmodel = s_task + LIN_TASK_CACHE * 6;   // [LIN2_CAMS]
  uint16_t* s_slot = reinterpret_cast<uint16_t*>(s_cmodel + LIN2_CAMS);   // [LIN2_PIECES] pair -> slot of its block record
  uint8_t* s_plm = reinterpret_cast<uint8_t*>(s_slot + LIN2_PIECES);      // [LIN2_PIECES] group-local landmark of a pair
  double* s_step = reinterpret_cast<double*>(s_lpb + LIN2_IDX_INTS);      // [step_doubles]: pose part of the step | fused: aux area
  double* s_aux = s_step + (step_doubles - Lin2Cfg<REAL, FUSE, UB>::MIN_STEP_DOUBLES);   // (fused: inverse landmark blocks, J^T J blocks, offsets)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
