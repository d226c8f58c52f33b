// Stand-alone driver for zh_zip_write_batch, zh_zip_create_batch and zh_zip_create under -fsanitize=address,undefined
// (built by tests/test_zip_write_sanitize.py from zippy_amd/csrc against the emulator runtime of tests/hipemu).  The
// directory holds what the test dumped:
//   calls.txt       "NAME N_ZIP N_ENTRIES TIME DATE" a line: one call of each batch form over the table, and one
//                   zh_zip_create an archive
//   NAME.tab        "ARCHIVE IS_DIRECTORY" a line, entry k's; NAME_<k>.path and NAME_<k>.data its path and contents
// and receives out.txt, "NAME FORM ARCHIVE STATUS LEN" a line (FORM: v1, v2, one), and NAME.FORM.<t>.img for every
// archive that was written.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/zippy_hip.h"

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static int bad = 0;
static FILE* out = nullptr;
static std::string dir;

static void report(const std::string& name, const char* form, size_t t, int status, void* img, size_t len, unsigned long* sum) {
  fprintf(out, "%s %s %zu %d %zu\n", name.c_str(), form, t, status, len);
  if ((status == ZH_OK) != (img != nullptr)) {
    fprintf(stderr, "%s %s archive %zu: status %d with%s an image\n", name.c_str(), form, t, status, img ? "" : "out");
    bad++;
  }
  if (img) {
    std::ofstream f(dir + "/" + name + "." + form + "." + std::to_string(t) + ".img", std::ios::binary);
    f.write((const char*)img, (std::streamsize)len);
    for (size_t j = 0; j < len; j++) *sum += ((const unsigned char*)img)[j];
  }
  zh_free(img);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  dir = argv[1];
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  out = fopen((dir + "/out.txt").c_str(), "w");
  if (!out) return 4;
  unsigned long sum = 0;
  std::ifstream calls(dir + "/calls.txt");
  std::string name;
  size_t n_zip, n_ent, n_calls = 0;
  unsigned time, date;
  while (calls >> name >> n_zip >> n_ent >> time >> date) {
    std::vector<std::string> paths(n_ent), datas(n_ent);
    std::vector<zh_zip_new_entry> tab(n_ent);
    std::vector<size_t> first(n_zip + 1, 0);
    std::ifstream f(dir + "/" + name + ".tab");
    for (size_t k = 0; k < n_ent; k++) {
      size_t t;
      int is_dir;
      f >> t >> is_dir;
      paths[k] = slurp(dir + "/" + name + "_" + std::to_string(k) + ".path");
      datas[k] = slurp(dir + "/" + name + "_" + std::to_string(k) + ".data");
      tab[k] = zh_zip_new_entry{paths[k].data(), paths[k].size(), datas[k].data(), datas[k].size(), is_dir,
                                (uint16_t)time, (uint16_t)date};
      first[t + 1]++;
    }
    for (size_t t = 0; t < n_zip; t++) first[t + 1] += first[t];
    std::vector<void*> dst(n_zip);
    std::vector<size_t> len(n_zip);
    std::vector<int32_t> st(n_zip);
    int rc = zh_zip_write_batch(ctx, tab.data(), first.data(), n_zip, ZH_DEFAULT_COMPRESSION, dst.data(), len.data(), st.data());
    if (rc) fprintf(stderr, "%s: zh_zip_write_batch %d\n", name.c_str(), rc), bad++;
    for (size_t t = 0; t < n_zip && !rc; t++) report(name, "v1", t, st[t], dst[t], len[t], &sum);
    rc = zh_zip_create_batch(ctx, tab.data(), first.data(), n_zip, ZH_BEST_SPEED, dst.data(), len.data(), st.data());
    if (rc) fprintf(stderr, "%s: zh_zip_create_batch %d\n", name.c_str(), rc), bad++;
    for (size_t t = 0; t < n_zip && !rc; t++) report(name, "v2", t, st[t], dst[t], len[t], &sum);
    for (size_t t = 0; t < n_zip; t++) {
      std::vector<const char*> p;
      std::vector<const void*> c;
      std::vector<size_t> pl, cl;
      for (size_t k = first[t]; k < first[t + 1]; k++) {
        p.push_back(tab[k].path);
        pl.push_back(tab[k].path_len);
        c.push_back(tab[k].contents);
        cl.push_back(tab[k].len);
      }
      void* img = nullptr;
      size_t n = 0;
      const size_t m = p.size();  // (no entries: NULL arrays)
      rc = zh_zip_create(ctx, m ? p.data() : nullptr, m ? pl.data() : nullptr, m ? c.data() : nullptr,
                         m ? cl.data() : nullptr, m, (uint16_t)time, (uint16_t)date, &img, &n);
      report(name, "one", t, rc, img, n, &sum);
    }
    n_calls++;
  }
  if (!n_calls) fprintf(stderr, "no calls\n"), bad++;
  fclose(out);
  zh_destroy(ctx);
  printf("%s: checksum %lu\n", bad ? "FAILED" : "sanitized zip writers ok", sum);
  return bad ? 1 : 0;
}
