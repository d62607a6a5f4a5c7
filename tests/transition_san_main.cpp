// transition_san_main.cpp — TEST ONLY: a program of its own around transition_harness.cpp,
// built with -fsanitize=address,undefined by tests/test_transition_cpu.py and run as a child
// process. Every array of the model and of the two data slots is a heap block of exactly
// its size, so a read or write past a field through the aliased pointers is reported.
//   transition_san MODEL EFC_CAP CON_CAP qpos... qvel... act... ctrl...
// MODEL (test_transition_cpu._dump_model): the sizes as int32 in MJHIP_MODEL_SIZES order,
// mjhipOption's bytes, then per array of MJHIP_MODEL_POINTERS an int64 count and the values.
// Prints the status and A (centred differences, eps 1e-6) as hexadecimal floats.
#include <stdio.h>

#include "transition_harness.cpp"

template <class T>
static T* readArray(FILE* f) {
  long long n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1) exit(3);
  if (n == 0) return nullptr;
  T* p = new T[n];
  if (fread(p, sizeof(T), (size_t)n, f) != (size_t)n) exit(3);
  return p;
}

struct Slot {
  mjhipData d{};
  ThSlot s{};
};

static void makeSlot(const mjhipModel* m, int efc_cap, int con_cap, Slot* out) {
  mjhipData& d = out->d;
#define MJ_M(n) m->n
#define XD(name, d0, d1, stage) d.name = new double[(m->d0) * (d1)]();
  MJHIP_DATA_FIELDS
  MJHIP_DATA_FORWARD
  MJHIP_DATA_ACTIVATION
  MJHIP_DATA_SENSOR_AUX
#undef XD
#undef MJ_M
  long nd, ni;
  kh_sizes(m, efc_cap, con_cap, &nd, &ni);
  out->s.d = &d;
  out->s.scratch = new double[nd]();
  out->s.iscratch = new int[ni]();
  out->s.step_scratch = new double[th_scratchDoubles(m) + 1]();
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  mjhipModel m{};
#define XS(name) if (fread(&m.name, sizeof(int), 1, f) != 1) return 3;
  MJHIP_MODEL_SIZES
#undef XS
  if (fread(&m.opt, sizeof(m.opt), 1, f) != 1) return 3;
#define X(type, name, d0, d1) m.name = readArray<type>(f);
  MJHIP_MODEL_POINTERS
#undef X
  fclose(f);
  const int efc_cap = atoi(argv[2]), con_cap = atoi(argv[3]);
  const int nstate = m.nq + m.nv + m.na, ndx = 2*m.nv + m.na;
  if (argc != 4 + nstate + m.nu) return 2;
  std::vector<double> x(nstate + m.nu + 1);
  for (int k = 0; k < nstate + m.nu; k++) x[k] = atof(argv[4 + k]);
  Slot centre, eval;
  makeSlot(&m, efc_cap, con_cap, &centre);
  makeSlot(&m, efc_cap, con_cap, &eval);
  const int P = th_slots(&m, 1, 1, 1);
  std::vector<double> Y((size_t)(1 + P)*nstate), A((size_t)ndx*ndx), B((size_t)ndx*m.nu + 1);
  int status = 0;
  const int rc = th_transition(&m, &centre.s, &eval.s, efc_cap, con_cap, x.data(),
                               x.data() + m.nq, m.na ? x.data() + m.nq + m.nv : nullptr,
                               m.nu ? x.data() + nstate : nullptr, nullptr, nullptr, 1e-6, 1, 3,
                               Y.data(), A.data(), m.nu ? B.data() : nullptr, &status);
  if (rc) return 4;
  printf("%a\n", (double)status);
  for (double v : A) printf("%a\n", v);
  return 0;
}
