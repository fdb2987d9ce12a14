function [pk,vk,ak,K_T_used,scene_status] = disturbedTransition(po,pf,prm,K_T_max,error_tol,noise_p,noise_v,seed,wind,pushes)
% Disturbed transition (no reference counterpart): the whole k-loop of dmpc_mex('transition', ..) with wind, noise and pushes added to the state of
% every commanded agent between the state advance and the history record of every column from 1 on -- the rule include/dmpc_hip.h pins.
% po: 3 x N (or 1 x 3 x N); pf: 3 x N_cmd, N_cmd <= N (the vehicles behind the commanded ones are static obstacles).  prm: a dmpc_params_struct.
% noise_p (metres), noise_v (m/s): half-widths of the uniform noise, default 0; seed: its stream, an integer below 2^53, default 0.
% wind (3 x 1, m/s^2, default []): a constant acceleration.  pushes (8 x n, default []): one push per column -- agent (1-based), history column
% (0-based as K_T_used counts them, >= 1), dp (3, metres), dv (3, m/s).
% pk, vk, ak (3 x K_T_max x N_cmd), K_T_used, scene_status: as 'transition'; the histories hold the disturbed states.
po = reshape(po,3,[]); pf = reshape(pf,3,[]);
if nargin < 6 || isempty(noise_p), noise_p = 0; end
if nargin < 7 || isempty(noise_v), noise_v = 0; end
if nargin < 8 || isempty(seed), seed = 0; end
if nargin < 9, wind = []; end
if nargin < 10, pushes = []; end
[pk,vk,ak,K_T_used,scene_status] = dmpc_mex('transition_disturbed', prm, po, pf, K_T_max, error_tol, noise_p, noise_v, seed, wind, pushes);
end
