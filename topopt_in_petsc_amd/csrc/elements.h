// elements.h -- host-side element matrices of the product (computed once per
// context).  Same formulas and accumulation order as the reference so that the
// matrices agree with it to the last bit (checked against tests/golden/ref_*.bin).
#pragma once
#include <cmath>
#include <cstring>

// 8-node isoparametric hexahedron, 2x2x2 Gauss, unit Young's modulus:
// KE = sum_gp w |J| B^T C B       (LinearElasticity.cc:841-998, redInt = 0)
inline void hex8_stiffness_box(double dx, double dy, double dz, double nu, double *ke /*576*/) {
    const double X[8] = {0.0, dx, dx, 0.0, 0.0, dx, dx, 0.0};
    const double Y[8] = {0.0, 0.0, dy, dy, 0.0, 0.0, dy, dy};
    const double Z[8] = {0.0, 0.0, 0.0, 0.0, dz, dz, dz, dz};
    const double sgx[8] = {-1, 1, 1, -1, -1, 1, 1, -1}, sgy[8] = {-1, -1, 1, 1, -1, -1, 1, 1},
                 sgz[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
    const double lambda = nu / ((1.0 + nu) * (1.0 - 2.0 * nu)), mu = 1.0 / (2.0 * (1.0 + nu));
    double C[6][6] = {};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) C[i][j] = lambda;
        C[i][i] = lambda + 2.0 * mu;
        C[i + 3][i + 3] = mu;
    }
    // engineering strain rows: xx, yy, zz, xy, yz, zx.  sel[d][row] = displacement
    // component whose d-derivative enters that row (-1: none)
    const int sel[3][6] = {{0, -1, -1, 1, -1, 2}, {-1, 1, -1, 0, 2, -1}, {-1, -1, 2, -1, 1, 0}};
    const double gp[2] = {-0.577350269189626, 0.577350269189626};
    std::memset(ke, 0, sizeof(double) * 576);
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++)
            for (int c = 0; c < 2; c++) {
                const double xi = gp[a], eta = gp[b], zeta = gp[c];
                double dN[3][8];
                for (int n = 0; n < 8; n++) {
                    dN[0][n] = (sgx[n] * 0.125) * (1.0 + sgy[n] * eta) * (1.0 + sgz[n] * zeta);
                    dN[1][n] = (sgy[n] * 0.125) * (1.0 + sgx[n] * xi) * (1.0 + sgz[n] * zeta);
                    dN[2][n] = (sgz[n] * 0.125) * (1.0 + sgx[n] * xi) * (1.0 + sgy[n] * eta);
                }
                double J[3][3];
                for (int r = 0; r < 3; r++) {
                    double sx = 0.0, sy = 0.0, sz = 0.0;
                    for (int n = 0; n < 8; n++) {
                        sx = sx + dN[r][n] * X[n];
                        sy = sy + dN[r][n] * Y[n];
                        sz = sz + dN[r][n] * Z[n];
                    }
                    J[r][0] = sx;
                    J[r][1] = sy;
                    J[r][2] = sz;
                }
                const double det = J[0][0] * (J[1][1] * J[2][2] - J[2][1] * J[1][2]) -
                                   J[0][1] * (J[1][0] * J[2][2] - J[2][0] * J[1][2]) +
                                   J[0][2] * (J[1][0] * J[2][1] - J[2][0] * J[1][1]);
                double iJ[3][3];
                iJ[0][0] = (J[1][1] * J[2][2] - J[2][1] * J[1][2]) / det;
                iJ[0][1] = -(J[0][1] * J[2][2] - J[0][2] * J[2][1]) / det;
                iJ[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
                iJ[1][0] = -(J[1][0] * J[2][2] - J[1][2] * J[2][0]) / det;
                iJ[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
                iJ[1][2] = -(J[0][0] * J[1][2] - J[0][2] * J[1][0]) / det;
                iJ[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) / det;
                iJ[2][1] = -(J[0][0] * J[2][1] - J[0][1] * J[2][0]) / det;
                iJ[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) / det;
                const double weight = 1.0 * 1.0 * 1.0 * det;
                double B[6][24] = {};
                for (int ll = 0; ll < 3; ll++) {
                    double beta[6][3];
                    for (int i = 0; i < 6; i++)
                        for (int j = 0; j < 3; j++)
                            beta[i][j] = iJ[0][ll] * (sel[0][i] == j ? 1.0 : 0.0) + iJ[1][ll] * (sel[1][i] == j ? 1.0 : 0.0) +
                                         iJ[2][ll] * (sel[2][i] == j ? 1.0 : 0.0);
                    for (int i = 0; i < 6; i++)
                        for (int j = 0; j < 24; j++) B[i][j] = B[i][j] + beta[i][j % 3] * dN[ll][j / 3];
                }
                for (int i = 0; i < 24; i++)
                    for (int j = 0; j < 24; j++)
                        for (int k = 0; k < 6; k++)
                            for (int l = 0; l < 6; l++) ke[j + 24 * i] = ke[j + 24 * i] + weight * (B[k][i] * C[k][l] * B[l][j]);
            }
}

// Von Mises form of the box element at its centroid: M = B0^T C^T Vm C B0 with B0 the 6 x 24 strain-displacement matrix
// at xi = eta = zeta = 0 (node order and strain rows xx, yy, zz, xy, yz, zx of hex8_stiffness_box, engineering shear),
// C the unit-modulus isotropic matrix built there and Vm the von Mises matrix (1 on the normal diagonal, -1/2 between
// normals, 3 on the shear diagonal):  u_e^T M u_e = sigma_vm^2 of the unit-modulus stress C B0 u_e.  Symmetric by
// construction (the two triangles are computed as one value); M annihilates rigid translations to rounding.
inline void hex8_vonmises_form_box(double dx, double dy, double dz, double nu, double *M /*576*/) {
    const double sg[3][8] = {{-1, 1, 1, -1, -1, 1, 1, -1}, {-1, -1, 1, 1, -1, -1, 1, 1}, {-1, -1, -1, -1, 1, 1, 1, 1}};
    const double hd[3] = {dx, dy, dz};
    const double lambda = nu / ((1.0 + nu) * (1.0 - 2.0 * nu)), mu = 1.0 / (2.0 * (1.0 + nu));
    double C[6][6] = {}, Vm[6][6] = {};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            C[i][j] = lambda;
            Vm[i][j] = -0.5;
        }
        C[i][i] = lambda + 2.0 * mu;
        C[i + 3][i + 3] = mu;
        Vm[i][i] = 1.0;
        Vm[i + 3][i + 3] = 3.0;
    }
    const int sel[3][6] = {{0, -1, -1, 1, -1, 2}, {-1, 1, -1, 0, 2, -1}, {-1, -1, 2, -1, 1, 0}};
    double B[6][24] = {};
    for (int d = 0; d < 3; d++)
        for (int row = 0; row < 6; row++)
            if (sel[d][row] >= 0)
                for (int n = 0; n < 8; n++) B[row][3 * n + sel[d][row]] = sg[d][n] / (4.0 * hd[d]);  // dN_n/dx_d at the centroid
    double S[6][24], W[6][24];  // S = C B0, W = Vm S
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 24; j++) {
            double s = 0.0;
            for (int k = 0; k < 6; k++) s += C[i][k] * B[k][j];
            S[i][j] = s;
        }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 24; j++) {
            double s = 0.0;
            for (int k = 0; k < 6; k++) s += Vm[i][k] * S[k][j];
            W[i][j] = s;
        }
    for (int i = 0; i < 24; i++)
        for (int j = i; j < 24; j++) {
            double s = 0.0;
            for (int k = 0; k < 6; k++) s += S[k][i] * W[k][j];
            M[24 * i + j] = M[24 * j + i] = s;
        }
}

// Helmholtz filter element matrix KF = R^2 int grad N . grad N + int N N on a
// box element, closed form (PDEFilter.cc:472-565); entries depend only on
// which axes the two nodes differ along.
inline void helmholtz_element_box(double dx, double dy, double dz, double RR, double *KF /*64*/) {
    const double pre1 = 1.0 / dx / dy, pre2 = 1 / dz;
    const double r2 = RR * RR, x2 = dx * dx, y2 = dy * dy, z2 = dz * dz;
    const double rx = r2 * x2;
    const double gxy = rx * y2, gxz = rx * z2, gyz = r2 * y2 * z2, mass = x2 * y2 * z2;
    const double a3 = 3.0 * gxy, b3 = 3.0 * gxz, c3 = 3.0 * gyz, a6 = 6.0 * gxy, b6 = 6.0 * gxz, c6 = 6.0 * gyz;
    double v[8];  // index = dx_differs + 2*dy_differs + 4*dz_differs
    v[0] = pre1 * pre2 * (a3 + b3 + c3 + mass) / 27.0;
    v[1] = pre1 * pre2 * (a3 + b3 - c6 + mass) / 54.0;
    v[3] = pre1 * pre2 * (a3 - b6 - c6 + mass) / 108.0;
    v[2] = pre1 * pre2 * (a3 - b6 + c3 + mass) / 54.0;
    v[4] = -(pre1 * pre2 * (a6 - b3 - c3 - mass) / 54.0);
    v[5] = -(pre1 * pre2 * (a6 - b3 + c6 - mass) / 108.0);
    v[7] = -(pre1 * pre2 * (a6 + b6 + c6 - mass) / 216.0);
    v[6] = -(pre1 * pre2 * (a6 + b6 - c3 - mass) / 108.0);
    const int lx[8] = {0, 1, 1, 0, 0, 1, 1, 0}, ly[8] = {0, 0, 1, 1, 0, 0, 1, 1}, lz[8] = {0, 0, 0, 0, 1, 1, 1, 1};
    for (int p = 0; p < 8; p++)
        for (int q = 0; q < 8; q++)
            KF[8 * p + q] = v[(lx[p] != lx[q]) + 2 * (ly[p] != ly[q]) + 4 * (lz[p] != lz[q])];
}

// Conduction element matrix KT = int grad N_a . grad N_b on a box element at unit conductivity, closed form: the tensor sum
// Sx (x) My (x) Mz + Mx (x) Sy (x) Mz + Mx (x) My (x) Sz of the 1-D stiffness S = [[1, -1], [-1, 1]] / h and mass
// M = h [[2, 1], [1, 2]] / 6 per axis -- the gradient part of helmholtz_element_box, (KF(R = 2) - KF(R = 1)) / 3.  Like KF its
// entries depend only on the axes along which the two corners differ: v8[dx + 2 dy + 4 dz] (optional) holds the 8 values.
inline void conduction_element_box(double dx, double dy, double dz, double *KT /*64*/, double *v8 = nullptr) {
    const double h[3] = {dx, dy, dz};
    double S[3][2], M[3][2];  // [axis][corners differ along it]
    for (int d = 0; d < 3; d++) {
        S[d][0] = 1.0 / h[d], S[d][1] = -1.0 / h[d];
        M[d][0] = h[d] / 3.0, M[d][1] = h[d] / 6.0;
    }
    double v[8];
    for (int q = 0; q < 8; q++) {
        const int x = q & 1, y = (q >> 1) & 1, z = q >> 2;
        v[q] = S[0][x] * M[1][y] * M[2][z] + M[0][x] * S[1][y] * M[2][z] + M[0][x] * M[1][y] * S[2][z];
    }
    const int lx[8] = {0, 1, 1, 0, 0, 1, 1, 0}, ly[8] = {0, 0, 1, 1, 0, 0, 1, 1}, lz[8] = {0, 0, 0, 0, 1, 1, 1, 1};
    for (int p = 0; p < 8; p++)
        for (int q = 0; q < 8; q++) KT[8 * p + q] = v[(lx[p] != lx[q]) + 2 * (ly[p] != ly[q]) + 4 * (lz[p] != lz[q])];
    if (v8)
        for (int q = 0; q < 8; q++) v8[q] = v[q];
}

// Thermoelastic coupling matrix G[(a,c), b] = 1 / (1 - 2 nu) int dN_a/dx_c N_b dV on a box element (24 x 8, row 3 a + c, row
// major): B^T D0 phi N_b integrated, D0 the unit-modulus isotropic matrix, phi = (1, 1, 1, 0, 0, 0).  A tensor product: along
// axis c the factor int dN_a/dx N_b = -+ 1/2 (the sign is corner a's side of the axis), along the two other axes the 1-D mass
// M_d = h_d [[2, 1], [1, 2]] / 6.  Nine magnitudes, g9[3 c + m] with m the number of the two other axes along which a and b
// differ (weights 4, 2, 1 of h_d1 h_d2 / 36) -- optional, what the kernels take as arguments.
inline void thermal_coupling_box(double dx, double dy, double dz, double nu, double *G /*192*/, double *g9 = nullptr) {
    const double h[3] = {dx, dy, dz};
    const double pre = 0.5 / (1.0 - 2.0 * nu);
    double m9[9];
    for (int c = 0; c < 3; c++) {
        const double area = h[(c + 1) % 3] * h[(c + 2) % 3];
        m9[3 * c + 0] = pre * (area / 9.0);
        m9[3 * c + 1] = pre * (area / 18.0);
        m9[3 * c + 2] = pre * (area / 36.0);
    }
    const int l[3][8] = {{0, 1, 1, 0, 0, 1, 1, 0}, {0, 0, 1, 1, 0, 0, 1, 1}, {0, 0, 0, 0, 1, 1, 1, 1}};
    for (int a = 0; a < 8; a++)
        for (int c = 0; c < 3; c++)
            for (int b = 0; b < 8; b++) {
                const int m = (l[(c + 1) % 3][a] != l[(c + 1) % 3][b]) + (l[(c + 2) % 3][a] != l[(c + 2) % 3][b]);
                G[(3 * a + c) * 8 + b] = l[c][a] ? m9[3 * c + m] : -m9[3 * c + m];
            }
    if (g9)
        for (int q = 0; q < 9; q++) g9[q] = m9[q];
}

// Tables of the geometric (stress) stiffness of the box element, design independent: at the 8 Gauss points of
// hex8_stiffness_box (same points, loop order a, b, c over xi, eta, zeta, same Jacobian and B accumulation) the physical
// shape-function gradients gradN[(3 gp + d) * 8 + n] = dN_n/dx_d, and the unit-modulus stress rows
// cb[(6 gp + r) * 24 + j] = (C0 B(gp))[r][j] (rows xx, yy, zz, xy, yz, zx; engineering shear in B).  The Gauss weight is
// dx dy dz / 8 for every point.
inline void hex8_geom_tables_box(double dx, double dy, double dz, double nu, double *gradN /*192*/, double *cb /*1152*/) {
    const double X[8] = {0.0, dx, dx, 0.0, 0.0, dx, dx, 0.0};
    const double Y[8] = {0.0, 0.0, dy, dy, 0.0, 0.0, dy, dy};
    const double Z[8] = {0.0, 0.0, 0.0, 0.0, dz, dz, dz, dz};
    const double sgx[8] = {-1, 1, 1, -1, -1, 1, 1, -1}, sgy[8] = {-1, -1, 1, 1, -1, -1, 1, 1},
                 sgz[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
    const double lambda = nu / ((1.0 + nu) * (1.0 - 2.0 * nu)), mu = 1.0 / (2.0 * (1.0 + nu));
    double C[6][6] = {};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) C[i][j] = lambda;
        C[i][i] = lambda + 2.0 * mu;
        C[i + 3][i + 3] = mu;
    }
    const int sel[3][6] = {{0, -1, -1, 1, -1, 2}, {-1, 1, -1, 0, 2, -1}, {-1, -1, 2, -1, 1, 0}};
    const double gp[2] = {-0.577350269189626, 0.577350269189626};
    int q = 0;
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++)
            for (int c = 0; c < 2; c++, q++) {
                const double xi = gp[a], eta = gp[b], zeta = gp[c];
                double dN[3][8];
                for (int n = 0; n < 8; n++) {
                    dN[0][n] = (sgx[n] * 0.125) * (1.0 + sgy[n] * eta) * (1.0 + sgz[n] * zeta);
                    dN[1][n] = (sgy[n] * 0.125) * (1.0 + sgx[n] * xi) * (1.0 + sgz[n] * zeta);
                    dN[2][n] = (sgz[n] * 0.125) * (1.0 + sgx[n] * xi) * (1.0 + sgy[n] * eta);
                }
                double J[3][3];
                for (int r = 0; r < 3; r++) {
                    double sx = 0.0, sy = 0.0, sz = 0.0;
                    for (int n = 0; n < 8; n++) {
                        sx = sx + dN[r][n] * X[n];
                        sy = sy + dN[r][n] * Y[n];
                        sz = sz + dN[r][n] * Z[n];
                    }
                    J[r][0] = sx;
                    J[r][1] = sy;
                    J[r][2] = sz;
                }
                const double det = J[0][0] * (J[1][1] * J[2][2] - J[2][1] * J[1][2]) -
                                   J[0][1] * (J[1][0] * J[2][2] - J[2][0] * J[1][2]) +
                                   J[0][2] * (J[1][0] * J[2][1] - J[2][0] * J[1][1]);
                double iJ[3][3];
                iJ[0][0] = (J[1][1] * J[2][2] - J[2][1] * J[1][2]) / det;
                iJ[0][1] = -(J[0][1] * J[2][2] - J[0][2] * J[2][1]) / det;
                iJ[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
                iJ[1][0] = -(J[1][0] * J[2][2] - J[1][2] * J[2][0]) / det;
                iJ[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
                iJ[1][2] = -(J[0][0] * J[1][2] - J[0][2] * J[1][0]) / det;
                iJ[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) / det;
                iJ[2][1] = -(J[0][0] * J[2][1] - J[0][1] * J[2][0]) / det;
                iJ[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) / det;
                double B[6][24] = {}, G[3][8] = {};
                for (int ll = 0; ll < 3; ll++) {
                    double beta[6][3];
                    for (int i = 0; i < 6; i++)
                        for (int j = 0; j < 3; j++)
                            beta[i][j] = iJ[0][ll] * (sel[0][i] == j ? 1.0 : 0.0) + iJ[1][ll] * (sel[1][i] == j ? 1.0 : 0.0) +
                                         iJ[2][ll] * (sel[2][i] == j ? 1.0 : 0.0);
                    for (int i = 0; i < 6; i++)
                        for (int j = 0; j < 24; j++) B[i][j] = B[i][j] + beta[i][j % 3] * dN[ll][j / 3];
                    for (int d = 0; d < 3; d++)
                        for (int n = 0; n < 8; n++) G[d][n] = G[d][n] + iJ[d][ll] * dN[ll][n];
                }
                for (int d = 0; d < 3; d++)
                    for (int n = 0; n < 8; n++) gradN[(3 * q + d) * 8 + n] = G[d][n];
                for (int r = 0; r < 6; r++)
                    for (int j = 0; j < 24; j++) {
                        double s = 0.0;
                        for (int k = 0; k < 6; k++) s = s + C[r][k] * B[k][j];
                        cb[(6 * q + r) * 24 + j] = s;
                    }
            }
}
