// solver_san_main.cpp — TEST ONLY: a program of its own around solver_harness.cpp, built with
// -fsanitize=address,undefined by tests/test_solver_cpu.py and run as a child process. Every
// array of the model, of the data, of the per-instance scratch (rows and contacts included)
// and of the solver scratch is a heap block of exactly its size, so a read or write past a
// field is reported.
//   solver_san MODEL EFC_CAP CON_CAP ITERATIONS LS_ITERATIONS TOLERANCE LS_TOLERANCE
//              MEANINERTIA qpos... qvel...
// MODEL (test_solver_cpu._dump_model): the sizes as int32 in MJHIP_MODEL_SIZES order,
// mjhipOption's bytes, then per array of MJHIP_MODEL_POINTERS an int64 count and the values.
// Prints the status, niter, qacc and qacc_smooth (hexadecimal floats).
#include <stdio.h>

#include "solver_harness.cpp"

template <class T>
static T* readArray(FILE* f) {
  long long n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1) exit(3);
  if (n == 0) return nullptr;
  T* p = new T[n];
  if (fread(p, sizeof(T), (size_t)n, f) != (size_t)n) exit(3);
  return p;
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  mjhipModel mm{};
#define XS(name) if (fread(&mm.name, sizeof(int), 1, f) != 1) return 3;
  MJHIP_MODEL_SIZES
#undef XS
  if (fread(&mm.opt, sizeof(mm.opt), 1, f) != 1) return 3;
#define X(type, name, d0, d1) mm.name = readArray<type>(f);
  MJHIP_MODEL_POINTERS
#undef X
  fclose(f);
  const mjhipModel* m = &mm;
  const int efc_cap = atoi(argv[2]), con_cap = atoi(argv[3]);
  SoOpt o;
  o.iterations = atoi(argv[4]);
  o.ls_iterations = atoi(argv[5]);
  o.tolerance = atof(argv[6]);
  o.ls_tolerance = atof(argv[7]);
  o.meaninertia = atof(argv[8]);
  const int nq = m->nq, nv = m->nv, nbody = m->nbody;
  (void)nbody;
  if (argc != 9 + nq + nv) return 2;

  mjhipData d{};
#define MJ_M(n) m->n
#define XD(name, d0, d1, stage) d.name = new double[(m->d0) * (d1)]();
  MJHIP_DATA_FIELDS
  MJHIP_DATA_FORWARD
  MJHIP_DATA_ACTIVATION
  MJHIP_DATA_SENSOR_AUX
#undef XD
#undef MJ_M
  for (int k = 0; k < nq; k++) d.qpos[k] = atof(argv[9 + k]);
  for (int k = 0; k < nv; k++) d.qvel[k] = atof(argv[9 + nq + k]);

  // the harness's lane over one lump of scratch, then every scratch field moved to a heap
  // block of its own
  long nd, ni;
  kh_sizes(m, efc_cap, con_cap, &nd, &ni);
  double* lump = new double[nd]();
  int* ilump = new int[ni]();
  mjh::Lane<1> L = bind(m, &d, lump, ilump, efc_cap, con_cap);
#define XSC(name, n) L.name.p = new double[(n)]();
  MJHIP_SCRATCH_FIELDS
#undef XSC
#define XSI(name, n) L.name.p = new int[(n)]();
  MJHIP_SCRATCH_INT_FIELDS
#undef XSI
  L.time.p = &d.time;
  L.gxpos = L.geom_xpos;
  L.ccdx = L.ccd.p;
  L.ccdxi = L.ccdi.p;
  if (mjh_needSubtreeVel(m)) {
    L.subtree_linvel.p = d.subtree_linvel;
    L.subtree_angmom.p = d.subtree_angmom;
  }
  if (mjh_needRnePost(m)) {
    L.cacc.p = d.cacc;
    L.cfrc_int.p = d.cfrc_int;
    L.cfrc_ext.p = d.cfrc_ext;
  }

  mjh::SolverScratch<1> sc;
  auto blk = [](long n) { return mjh::SP<1>{new double[n]()}; };
  sc.L = blk((long)nv*nv);
  sc.Ma = blk(nv);
  sc.Mv = blk(nv);
  sc.grad = blk(nv);
  sc.Mgrad = blk(nv);
  sc.search = blk(nv);
  sc.vec = blk(nv);
  sc.qacc_warmstart = blk(nv);
  sc.efc_b = blk(efc_cap);
  sc.Jaref = blk(efc_cap);
  sc.Jv = blk(efc_cap);
  sc.D = blk(efc_cap);
  sc.quad = blk(3L*efc_cap);
  sc.oldstate.p = new int[efc_cap]();

  SoOut out{};
  std::vector<double> act3(3*(size_t)m->na + 1);
  const int st = soRun(m, &d, L, sc, m->na ? act3.data() : nullptr, &o, nullptr, 0, &out);
  printf("%d\n%d\n", st, out.niter);
  for (int k = 0; k < nv; k++) printf("%a\n", d.qacc[k]);
  for (int k = 0; k < nv; k++) printf("%a\n", d.qacc_smooth[k]);
  return 0;
}
